"""The fused Poisson operator on 3-D Q1 meshes (csrc/poisson3d_q1.inl, built three times through poisson3d_q1_g2/3/4.hip, and
csrc/poisson3d_q1_cf.hip): the five kernel families 3d_q1_cfz, 3d_q1_n2, 3d_q1_n1, 3d_q1_t16 and 3d_q1_generic against the float64 restatement
of dn_poisson_apply (poisson3d_ref.py), node by node, on every template instantiation the host can pick (part 1: the full product behind
launch3_flags, launch3_one, launch3_f32n, launch3_n2, launch3_n2_bc and launch_cf3_bc, at 34 x 17 x 6 and 33 x 17 x 6 nodes, B = 2, under
"PLAN3D" overrides that give two chunks, two tiles and two strips, the last one shorter) and on every launch seam (part 2: one element, one
layer, full and nearly empty chunks and tiles, three chunks, T16 tiles of 4, 8 and 12 rows, a generic tile whose width is no power of two,
workgroup counts below 8, a multiple of 8 and neither, strips of one layer, split launches, deferred sums, shared and per-sample arrays).

No tolerance is chosen.  For every free node e = |got - ref64| / (|out_scale| S_a), S_a the sum of |W_g t| over the placed terms (one per element and Gauss
point) that make up the node's value in the float64 restatement; where S_a == 0 the output is exactly 0; Dirichlet nodes are exactly 0.  A case
passes if max e <= K = 4 Y, Y being the largest e the float32 CPU evaluation of the same restatement reaches over all the cases of this file
with the same rule and forcing form -- measured against the reference alone, once per session.  Before every launch dn_poisson_query is
asked, and its family and geometry must be what the Python mirror of poisson_choose / plan3d_env says.

The scalars (poisson3d_ref.scalar_bounds, with the derivations):
    sumsq                       2 K sum |raw64| S + (R + 4) 2^-24 sumsq64   (t^2 added in fp32 per thread over the R + 1 planes of a strip)
    E2, E1 of per-point forms   n 2^-24 SE,  n = R + 2 + points of an element (27 stencil terms in 3d_q1_cfz) + 16   (chain_length)
    E1 of nodal-value forms     ((K + (R + 5) 2^-24) SN + |beta| (n + 3) 2^-24 SE2) / |alpha|     (3d_q1_cfz and every FL3_E1G instantiation:
                                e1 = ((sum_a u~_a t_a) / esc + beta e2) / alpha per thread, t_a within K S_a of float64)
energy_f32 is the float32 rounding of energy * energy_scale, exactly.

Yardsticks Y in units of 2^-24 (recomputed in every session; the float32 CPU arithmetic of another machine may move them by a unit or so):
    rule       forcing absent   nodal   at Gauss points   load vector
    2 points   8.98             9.41    9.45              8.85
    3 points   15.1             16.1    14.3              -
    4 points   23.3             22.4    21.9              -
What the MI355X gave, per family: the largest e / Y (the bound is 4) and the largest scalar error over its bound, with the case (every case
prints its own; run with -s):
    family          e / Y   at                                             energy   at                        sumsq    at
    3d_q1_cfz       1.04    2 points, f, one fp32 image                    0.0046   nu, box + fp32 image      0.014    32 x 16 x 2, nu, f, two fp32 images
    3d_q1_n2        1.13    rule (-0.5, 0.7), nu, one fp32 image, no sums  0.018    rule (-0.5, 0.7), nu,     0.027    rule (-0.5, 0.7), nu, load vector,
                                                                                    box + uint8 image                  box + uint8 image
    3d_q1_n1        1.34    weights (0.5, 1.5), f, two fp32 images         0.032    4 points, nu              0.027    4 points, nu, f, two fp32 images
    3d_q1_t16       0.92    weights (0.5, 1.5), nu, f at Gauss points      0.032    4 points, nu, f, general  0.027    4 points, nu, f_gp, general
    3d_q1_generic   1.27    weights (0.5, 1.5), nu, f                      0.032    4 points, nu, general     0.028    4 points, nu, f_gp, general
No family comes near the margin of 4, the closed form in z included: no form needed a count of roundings of its own in place of 4 Y.  The
scalars stay below a twentieth of their bounds.  The split launches add up to the single launch bitwise for 1, 2, 3 and 4 strips, the deferred
sums are bitwise the in-kernel reduction's, every sample of the B = 3 launches is bitwise its B = 1 launch, "PLAN3D" strip heights and (t16, generic) tile shapes
change no bit of `out`, dn_poisson_query agreed with the mirror on every launch, and at fp32 mask values of 0.5 and its two neighbours every kernel
does what dn_dirichlet says (`> 0.5`): no kernel needed a change.  One instantiation the kernel template allows cannot be reached
(test_the_one_instantiation_the_host_cannot_reach: FL3_E1G with fp32 images in the one-element node-owner form).
The offset case (u = 8 + rnd / 8, 34 x 17 x 6, B = 2, nu, nodal f, no condition: a Dirichlet value near 0 would put jumps of 8 into the field),
energy64 = 790.712 = c E1 - E2 = 771.220 + 19.492:
    SN / (alpha SE1) = 310.5;  |energy - ref64| = 1.5e-4 on 3d_q1_cfz (nodal values) and 3.4e-5 under "Q1_3D_E1SUM" (3d_q1_n2, point by point)
    -- 1.8e-4 of the nodal-value bound and 4.3e-4 of the per-point bound; the nodal-value form also stays inside the per-point bound (1.1e-3 of
    it): its error scale SN / alpha is 310 times the per-point one, its error here 4.4 times.
"""
import ctypes as C
import math

import numpy as np
import pytest

import poisson3d_ref as p
from poisson3d_ref import Case, K_of, build, choose, evaluate, node_error, reference
from q1_residual_ref import MARGIN, U

RATIOS = {}


# ---------------------------------------------------------------------------------------------
# running a case on the GPU
# ---------------------------------------------------------------------------------------------
def _geom(c):
    from diffnet_amd.fem import FemGeometry
    gx, gw = p.rule_points(c["rule"])
    return FemGeometry(3, c["mesh"], p.HS, 1, c["ngp"], gx, gw)


def _cu(a):
    from test_gpu_parity import cu
    return cu(a).unsqueeze(1)


class Switches:
    """the case's switches and "PLAN3D" for the duration of a block; everything is cleared afterwards"""
    KEYS = ("Q1_3D_E1", "Q1_3D_T16", "Q1_3D_N2", "Q1_3D_E1SUM", "PLAN3D")

    def __init__(self, c, plan=None):
        self.set = dict(c["switches"], PLAN3D=c["plan"] if plan is None else plan)

    def __enter__(self):
        from diffnet_amd import _lib, ops
        for k in self.KEYS:
            _lib.config_set(k, self.set.get(k, ""))
        ops.call_cache_clear()

    def __exit__(self, *exc):
        from diffnet_amd import _lib, ops
        for k in self.KEYS:
            _lib.config_set(k, "")
        ops.call_cache_clear()


def query(plan):
    from diffnet_amd import _lib
    k = _lib.DnPoissonKernel()
    rc = _lib.lib().dn_poisson_query(C.byref(plan.mesh), C.byref(plan.args), C.byref(k))
    return rc, k


def assert_query(c, plan, override=None, strip_select=0):
    """dn_poisson_query of the prepared launch against the Python mirror: family and geometry"""
    fam, g = choose(c, plan=override, strip_select=strip_select)
    rc, k = query(plan)
    assert rc == 0, (c["case"], rc)
    got = (p.FAM.get(k.family), k.tile[0], k.tile[1], k.E, k.R, k.chunks, k.tiles, k.strips, k.launched_strips, int(k.launched))
    want = (fam, g["TX"], g["TY"], g["E"], g["R"], g["chunks"], g["tiles"], g["strips"], g["launched_strips"], g["launched"])
    assert got == want, (c["case"], override, got, want)
    return fam, g


def prepare(c, override=None, strip_select=0, continues=None, pipelined=False, want_sums=None):
    """the PoissonPlan of a case (under the switches the caller holds), its outputs filled with sentinels: NaN in out, -1 in the scalars"""
    import torch
    from diffnet_amd import ops
    dl = []
    for m in c["conds"]:
        v = _cu(m["value"]) if isinstance(m["value"], np.ndarray) else m["value"]
        dl.append((ops.BoxFaces([n for n, b in p.FACES.items() if m["faces"] & b]) if m["kind"] == "box" else _cu(m["img"]), v))
    f = fgp = None
    if c["fkind"] == "gp":
        from test_gpu_parity import cu
        fgp = cu(c["f"])
    elif c["fkind"] == "nodal":
        f = _cu(c["f"])
    elif c["fkind"] == "load":
        f = ops.LoadVector(_cu(c["f"]))
    u = _cu(c["u"])
    ws = c["want_sums"] if want_sums is None else want_sums
    out = None if continues is not None else torch.full_like(u, float("nan"))
    pl = ops.PoissonPlan(_geom(c), u, None if c["nu"] is None else _cu(c["nu"]), f, fgp, dl, c["alpha"], c["beta"], c["c"], c["wscale"], c["out_scale"],
                         want_out=True, want_sums=ws, loss_scale=c["energy_scale"] if ws else None, out=out, strict=True, strip_select=strip_select,
                         continues=continues, pipelined_sums=pipelined)
    if ws and continues is None:
        pl.result[1].fill_(-1.0)
        pl.result[2].fill_(-1.0)
    assert_query(c, pl, override, strip_select)
    return pl


def fetch(pl):
    import torch
    torch.cuda.synchronize()
    out = pl.result[0].cpu().numpy()[:, 0]
    if pl.result[1] is None:
        return out, None, None, None
    s = pl.result[1].cpu().numpy()
    return out, float(s[0]), float(s[1]), pl.result[2].cpu().numpy().reshape(()).copy()


def launch(c, override=None, **kw):
    with Switches(c, override):
        pl = prepare(c, override, **kw)
        pl.launch()
        return fetch(pl)


def judge(c, ref, fam, g, got, label, nodes=True):
    """every figure of one launch against its bound; returns the lines that failed (all are printed first).  nodes=False: the node ratio is
    printed and not judged (the offset case, whose subject is the energy)"""
    out, energy, sumsq, ef32 = got
    B = c["B"]
    ngp, form = c["ngp"], p.forcing_form(c)
    Y = p.yardsticks()[(ngp, form)][0]
    K = MARGIN * Y
    bad = []
    assert out.dtype == np.float32 and out.shape == (B, *c["shape"])
    e, at = node_error(out, ref, c["out_scale"])
    line = f"p3-ratio {label} {fam} ngp={ngp} f={form}: e/Y = {e / Y:.3g} at {at} (Y = {Y / U:.3g} x 2^-24)"
    r = RATIOS.setdefault(fam, dict(e=(0.0, None), energy=(0.0, None), sumsq=(0.0, None)))
    if nodes and e / Y > r["e"][0]:
        r["e"] = (e / Y, label)
    if nodes and not e <= K:
        bad.append(line)
    if energy is not None:
        nodal = fam == "cfz" or "E1G" in p.selectors(c)[2]
        be, bs = p.scalar_bounds(c, ref, g, fam, nodal)
        ee, es = abs(energy - ref["energy"]), abs(sumsq - ref["sumsq"])
        re = ee / be if be > 0 else float(ee != 0)
        rs = es / bs if bs > 0 else float(es != 0)
        exact = np.float32(energy * c["energy_scale"]) == ef32
        line += (f" energy err/bound = {re:.3g} ({'nodal' if nodal else 'per-point'} E1) sumsq err/bound = {rs:.3g} "
                 f"energy_f32 {'exact' if exact else 'NOT the rounding'}")
        if re > r["energy"][0]:
            r["energy"] = (re, label)
        if rs > r["sumsq"][0]:
            r["sumsq"] = (rs, label)
        if not (re <= 1 and rs <= 1 and exact and math.isfinite(energy) and math.isfinite(sumsq)):
            bad.append(line)
    print(line)
    return bad


def check(case):
    c, ref = build(case), reference(case)
    fam, g = choose(c)
    return judge(c, ref, fam, g, launch(c), f"{case.rule} {case.base or '-'} {case.cond} {case.mesh} B={case.B} plan={case.plan or 'default'} {case.route}")


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("family", p.FAMILIES)
def test_every_instantiation_the_dispatch_can_pick(family, part):
    """part 1: the matrix of one family (coverage: test_matrix_is_the_full_product), in four parts"""
    cases = p.part1_cases(family)[part::4]
    bad = [b for case in cases for b in check(case)]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(p.SEAMS)), ids=lambda k: "x".join(map(str, p.SEAMS[k][0])) + f"-B{p.SEAMS[k][1]}-{p.SEAMS[k][2]}-{p.SEAMS[k][4]}")
def test_every_launch_seam(k):
    """part 2: one seam mesh (what it reaches: test_seam_list_reaches_every_seam)"""
    bad = check(p.part2_cases()[k])
    assert not bad, "\n".join(bad)


STRIP_FORMS = [("cfz", "g2", "16,16,2,{}", "sums"), ("n2", "g2", "16,16,2,{}", "n2"), ("n1", "g2", "16,16,1,{}", "sums"), ("t16", "w2", "16,8,1,{}", "sums")]


def _strip_case(fam, rule, plan, route, R):
    return Case("strips", rule, "NF", "u8x2", (34, 17, 9), 2, plan.format(R), route, 700)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [8, 4, 3, 2], ids=lambda R: f"R{R}")
@pytest.mark.parametrize("form", STRIP_FORMS, ids=lambda f: f[0])
def test_split_and_deferred_launches(form, R):
    """1, 2, 3 and 4 strips of 8 layers (R = 3: a shorter last strip).  strip_select 1 then 2 (accumulate_sums) into one NaN-filled `out`: the
    union is bitwise the single launch's `out`, the sums stay within their bound; defer_sums + dn_poisson_finish_sums gives bitwise the sums
    of the in-kernel reduction."""
    case = _strip_case(*form, R)
    c, ref = build(case), reference(case)
    fam, g = choose(c)
    assert fam == form[0] and g["strips"] == {8: 1, 4: 2, 3: 3, 2: 4}[R]
    whole = launch(c)
    bad = judge(c, ref, fam, g, whole, f"whole {fam} R={R}")
    with Switches(c):
        first = prepare(c, strip_select=1)
        first.launch()
        second = prepare(c, strip_select=2, continues=first)
        second.launch()
        split = fetch(second)
        deferred = prepare(c, pipelined=True)
        deferred.launch()
        deferred.finish_sums()
        late = fetch(deferred)
    assert np.array_equal(split[0].view(np.uint32), whole[0].view(np.uint32)), "the two launches of the split evaluation do not add up to the single launch, bitwise"
    bad += judge(c, ref, fam, g, split, f"split {fam} R={R}")
    assert np.array_equal(late[0].view(np.uint32), whole[0].view(np.uint32))
    assert (late[1], late[2], float(late[3])) == (whole[1], whole[2], float(whole[3])), ("deferred sums are not the in-kernel reduction's", late[1:], whole[1:])
    assert not bad, "\n".join(bad)


BATCH_FORMS = [("cfz", "g2", p.MESH_E, "16,16,2,3", "sums"), ("n2", "g2", p.MESH_E, "16,16,2,3", "n2"), ("n1", "g3", p.MESH_O, "16,16,1,3", "sums"),
               ("t16", "g2", p.MESH_O, "16,8,1,3", "sums"), ("generic", "g4", p.MESH_O, "32,8,1,3", "sums")]


@pytest.mark.gpu
@pytest.mark.parametrize("form", BATCH_FORMS, ids=lambda f: f[0])
def test_batch_of_three_with_shared_arrays(form):
    """B = 3 with nu, f and the first mask shared, the second mask per sample: sample b of `out` is bitwise what B = 1 gives for that sample"""
    fam, rule, mesh, plan, route = form
    case = Case("batch", rule, "NF", "u8x2", mesh, 3, plan, route, 3)
    c, ref = build(case), reference(case)
    assert c["nu"].shape[0] == 1 and c["f"].shape[0] == 1 and c["conds"][0]["img"].shape[0] == 1 and c["conds"][1]["img"].shape[0] == 3
    f3, g = choose(c)
    assert f3 == fam
    whole = launch(c)
    bad = judge(c, ref, fam, g, whole, f"batch {fam}")
    for b in range(3):
        one = dict(c, B=1, u=c["u"][b:b + 1], conds=[dict(m, img=m["img"][b:b + 1] if m["img"].shape[0] > 1 else m["img"]) for m in c["conds"]])
        assert choose(one)[0] == fam
        got = launch(one)[0]
        assert np.array_equal(got[0].view(np.uint32), whole[0][b].view(np.uint32)), (fam, b)
    assert not bad, "\n".join(bad)


OVERRIDES = [("cfz", "g2", (34, 17, 9), "sums", ["16,16,2,1", "16,16,2,3", "16,16,2,8"]), ("n2", "g2", (34, 17, 9), "n2", ["16,16,2,1", "16,16,2,3", "16,16,2,8"]),
             ("n1", "g2", (33, 16, 9), "sums", ["16,16,1,1", "16,16,1,3", "16,16,1,8"]), ("t16", "g2", (33, 17, 9), "sums", ["16,12,1,1", "16,12,1,8", "16,8,1,3", "16,4,1,3", "16,16,1,3"]),
             ("generic", "g3", (23, 11, 9), "sums", ["23,11,1,1", "23,11,1,3", "32,8,1,3", "64,4,1,3", "12,16,1,3"])]


def _override_case(form):
    fam, rule, mesh, route, _ = form
    return Case("override", rule, "NF" if fam != "generic" else "NG", "u8x2" if fam in ("cfz", "n2", "n1") else "general", mesh, 2, "", route, 800)


def test_plan_overrides_keep_the_family_and_change_the_plan():
    """by the mirror: every override of test_plan_overrides_change_no_bit_of_out stays in the default plan's family and changes its geometry"""
    for form in OVERRIDES:
        c = build(_override_case(form))
        f0, g0 = choose(c)
        assert f0 == form[0]
        for plan in form[4]:
            f1, g1 = choose(c, plan=plan)
            assert f1 == f0 and g1["E"] == g0["E"] and (g1["TX"], g1["TY"], g1["R"]) != (g0["TX"], g0["TY"], g0["R"]), (plan, g0, g1)


@pytest.mark.gpu
@pytest.mark.parametrize("form", OVERRIDES, ids=lambda f: f[0])
def test_plan_overrides_change_no_bit_of_out(form):
    """strips of 1, 3 and 8 layers through "PLAN3D" against the default plan's strips and, where the family has more than one tile shape (t16,
    generic), other tiles: `out` is bitwise the default plan's"""
    fam, plans = form[0], form[4]
    c = build(_override_case(form))
    base = launch(c)[0]
    for plan in plans:
        got = launch(c, override=plan)[0]
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (fam, plan)


@pytest.mark.gpu
def test_offset_field_on_the_nodal_value_energy():
    """u = 8 + rnd / 8: the stiffness energy from the finished nodal values (3d_q1_cfz) and summed point by point ("Q1_3D_E1SUM") on the same
    arguments.  Both are held to their own bound; SN / (alpha SE1), the factor by which the nodal-value form's error scale exceeds the
    per-point form's, is printed beside the two errors."""
    bad = []
    for case in p.offset_cases():
        c, ref = build(case), reference(case)
        fam, g = choose(c)
        assert fam == ("n2" if "e1sum" in case.route else "cfz")
        got = launch(c)
        bad += judge(c, ref, fam, g, got, f"offset {fam}", nodes=False)
        n = p.chain_length(c, g, fam)
        per_point = n * U * (abs(c["c"]) * ref["SE1"] + ref["SE2"])
        print(f"p3-offset {fam}: SN / (alpha SE1) = {ref['SN'] / (c['alpha'] * ref['SE1']):.4g}; |energy - ref64| = {abs(got[1] - ref['energy']):.4g} = "
              f"{abs(got[1] - ref['energy']) / per_point:.3g} x the per-point bound ({per_point:.4g}); energy64 = {ref['energy']:.9g}, "
              f"c E1 = {c['c'] * ref['E1']:.6g}, E2 = {ref['E2']:.6g}")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_zz_print_the_largest_ratio_of_every_family():
    """last in the file: the table the module docstring records (empty entries when the tests above were deselected)"""
    for fam in p.FAMILIES:
        r = RATIOS.get(fam)
        print(f"p3-family {fam}: " + ("not run" if r is None else f"largest e / Y = {r['e'][0]:.3g} at [{r['e'][1]}]; largest energy err / bound = "
                                      f"{r['energy'][0]:.3g} at [{r['energy'][1]}]; largest sumsq err / bound = {r['sumsq'][0]:.3g} at [{r['sumsq'][1]}]"))


# ---------------------------------------------------------------------------------------------
# CPU: the matrix, the mirror, the seam list, the reference, the yardstick, the comparator's teeth
# ---------------------------------------------------------------------------------------------
NKERN = dict(cfz={2: 48, 3: 0, 4: 0}, n2={2: 96, 3: 0, 4: 0}, n1={2: 52, 3: 20, 4: 20}, t16={2: 36, 3: 18, 4: 18}, generic={2: 36, 3: 18, 4: 18})


@pytest.mark.parametrize("family", p.FAMILIES)
def test_matrix_is_the_full_product(family):
    """the selector tuple of every part-1 argument set, derived from the arguments by the host's rules, covers the full product behind the
    launch functions; every case reaches the family it names, by the mirror alone; shared and per-sample arrays both occur"""
    cases = p.part1_cases(family)
    assert len(cases) == dict(cfz=48, n2=96, n1=100, t16=72, generic=72)[family] and len(set(cases)) == len(cases)
    built = [build(x) for x in cases]
    for c in built:
        assert choose(c)[0] == family, c["case"]
        assert c["B"] == 2 and c["mesh"] in (p.MESH_E, p.MESH_O)
        g = choose(c)[1]
        want = (3 if family in ("n1", "t16") else 2, 3 if family in ("t16", "generic") else 2, 2, 3)          # 16-wide one-element tiles: three chunks
        assert (g["chunks"], g["tiles"], g["strips"], g["R"]) == want, (c["case"], g)
    for ngp in (2, 3, 4):
        got = {p.selectors(c) for c in built if c["ngp"] == ngp}
        want = p.expected_kernels(family, ngp)
        assert len(want) == NKERN[family][ngp] and got == want, (family, ngp, sorted(map(str, got ^ want)))
    batched = lambda xs: {x.shape[0] > 1 for x in xs if isinstance(x, np.ndarray)}          # noqa: E731
    assert batched(c["nu"] for c in built) == {False, True}
    assert batched(c["f"] for c in built) == {False, True}
    assert batched(m.get("img") for c in built for m in c["conds"]) == {False, True}
    if family in ("t16", "generic"):
        assert batched(m["value"] for c in built for m in c["conds"]) == {False, True}
    if family in ("cfz", "n2"):
        assert {m["faces"] for c in built for m in c["conds"] if m["kind"] == "box"} == {63, 1 | 8 | 32}
        assert {tuple(m["kind"] for m in c["conds"]) for c in built} >= {("box", "u8"), ("u8", "box"), ("box", "f32"), ("f32", "box")}
    if family == "n2":
        routes = {(c["rule"], c["case"].route) for c in built}
        assert routes == {("g2", "n2"), ("u2", "sums"), ("u2", "nosums"), ("g2", "n2+nosums"), ("g2", "alpha0"), ("g2", "e1sum")}
        N = p.tables("u2")[0]
        assert abs(N[0, 1] + N[1, 1] - 1.0) > 1e-6                 # the branch of poisson_choose no other test takes
    if family in ("n1", "t16", "generic"):
        assert {c["rule"] for c in built} == {"g2", "w2", "g3", "g4"}
        assert not all(x == 1.0 for x in p.tables("w2")[2])


def test_the_one_instantiation_the_host_cannot_reach():
    """A finding: poisson3d_q1n_kernel could carry FL3_E1G together with fp32 mask images (FL3_BC_F32), but launch3_f32n never asks for it --
    with fp32 images the one-element node-owner form always sums the stiffness energy point by point, also where launch3_one would take it
    from the nodal values.  The matrix therefore holds 52 and not 60 two-point N1 instantiations; this test fails when the host changes."""
    cases = [build(x) for x in p.part1_cases("n1") if x.rule == "g2" and x.route.startswith("sums") and x.cond.startswith("f32")]
    assert len(cases) == 8
    for c in cases:
        fl = p.selectors(c)[2]
        assert "F32" in fl and "E1G" not in fl
    assert not any("E1G" in s[2] and "F32" in s[2] for s in p.expected_kernels("n1", 2))


def _fake_args(c, strip_select=0):
    """dn_mesh and dn_poisson_args of a case for dn_poisson_query, which follows no pointer: every array is a distinct 256-byte aligned address"""
    from diffnet_amd import _lib
    mesh = _geom(c).mesh_struct(c["B"])
    a = _lib.DnPoissonArgs()
    ptr = iter(range(1 << 20, 1 << 30, 1 << 20))
    a.u, a.out = next(ptr), next(ptr)
    if c["nu"] is not None:
        a.nu, a.nu_batched = next(ptr), int(c["nu"].shape[0] > 1)
    if c["fkind"] == "gp":
        a.f_gp = next(ptr)
    elif c["fkind"] is not None:
        a.f, a.f_is_load = next(ptr), int(c["fkind"] == "load")
    for k, m in enumerate(c["conds"]):
        bc = a.bc[k]
        if m["kind"] == "box":
            bc.mask_kind, bc.box_faces = _lib.MASK_BOX, m["faces"]
        else:
            bc.mask, bc.mask_kind = next(ptr), _lib.MASK_U8 if m["kind"] == "u8" else _lib.MASK_F32
        if isinstance(m["value"], np.ndarray):
            bc.field = next(ptr)
    a.alpha, a.beta, a.c, a.wscale, a.out_scale = c["alpha"], c["beta"], c["c"], c["wscale"], c["out_scale"]
    if c["want_sums"]:
        a.energy, a.sumsq, a.energy_f32, a.workspace, a.workspace_bytes = next(ptr), next(ptr), next(ptr), next(ptr), 1 << 30
    a.strip_select = strip_select
    return mesh, a


def test_the_mirror_is_the_library_choice():
    """dn_poisson_query needs no device: family and geometry of every case of the file, under the case's switches, against the Python mirror
    (the GPU tests ask again with the real arguments before every launch)"""
    from diffnet_amd import _lib
    others = [_strip_case(*f, R) for f in STRIP_FORMS for R in (8, 4, 3, 2)] + p.offset_cases() + \
        [Case("batch", rule, "NF", "u8x2", mesh, 3, plan, route, 3) for _, rule, mesh, plan, route in BATCH_FORMS]
    seen = set()
    try:
        for case in p.all_cases() + others:
            c = build(case)
            for k in Switches.KEYS:
                _lib.config_set(k, dict(c["switches"], PLAN3D=c["plan"]).get(k, ""))
            for sel in (0, 1, 2):
                fam, g = choose(c, strip_select=sel)
                mesh, a = _fake_args(c, sel)
                k = _lib.DnPoissonKernel()
                rc = _lib.lib().dn_poisson_query(C.byref(mesh), C.byref(a), C.byref(k))
                got = (rc, p.FAM.get(k.family), k.tile[0], k.tile[1], k.E, k.R, k.chunks, k.tiles, k.strips, k.launched_strips, int(k.launched))
                want = (0, fam, g["TX"], g["TY"], g["E"], g["R"], g["chunks"], g["tiles"], g["strips"], g["launched_strips"], g["launched"])
                assert got == want, (case, sel, got, want)
            seen.add(fam)
    finally:
        for k in Switches.KEYS:
            _lib.config_set(k, "")
    assert seen == set(p.FAMILIES)             # no family is unreachable


def test_seam_list_reaches_every_seam():
    """by the plan mirror alone: what the part-2 meshes reach, per kernel group (two-element forms, node-owner one-element form, w forms)"""
    rows = [(c, *choose(c)) for c in (build(x) for x in p.part2_cases())]
    for fam in ("cfz", "n2"):
        mine = [(c, g) for c, f, g in rows if f == fam]
        half = lambda c: c["mesh"][0] // 2                  # noqa: E731
        seen = dict(one_element=any(c["mesh"] == (2, 2, 2) for c, g in mine), one_layer=any(c["mesh"] == (32, 16, 2) for c, g in mine),
                    two_layers=any(c["mesh"] == (32, 16, 3) for c, g in mine),
                    half16=any(half(c) == 16 and g["chunks"] == 1 for c, g in mine), half17=any(half(c) == 17 and g["chunks"] == 2 for c, g in mine),
                    half31=any(half(c) == 31 and g["chunks"] == 2 for c, g in mine), three_chunks=any(g["chunks"] == 3 for c, g in mine),
                    ny16=any(c["mesh"][1] == 16 and g["tiles"] == 1 for c, g in mine), ny17=any(c["mesh"][1] == 17 and g["tiles"] == 2 for c, g in mine),
                    R1=any(g["R"] == 1 and g["strips"] > 1 for c, g in mine), R_not_dividing=any((c["mesh"][2] - 1) % g["R"] for c, g in mine),
                    wg_below_8=any(g["launched"] < 8 for c, g in mine), wg_multiple_of_8=any(g["launched"] % 8 == 0 for c, g in mine),
                    wg_neither=any(g["launched"] > 8 and g["launched"] % 8 for c, g in mine), default_plan=any(c["plan"] == "" for c, g in mine),
                    box=any(m["kind"] == "box" for c, g in mine for m in c["conds"]), load=any(c["fkind"] == "load" for c, g in mine))
        assert all(seen.values()), (fam, [k for k, v in seen.items() if not v])
    n1 = [(c, g) for c, f, g in rows if f == "n1"]
    seen = dict(nx16=any(c["mesh"][0] == 16 for c, g in n1), nx17=any(c["mesh"][0] == 17 and g["chunks"] == 2 for c, g in n1),
                nx31=any(c["mesh"][0] == 31 and g["chunks"] == 2 for c, g in n1), ny16=any(c["mesh"][1] == 16 for c, g in n1),
                ny31=any(c["mesh"][1] == 31 and g["tiles"] == 2 for c, g in n1), R1=any(g["R"] == 1 and g["strips"] > 1 for c, g in n1),
                rules={c["rule"] for c, g in n1} >= {"g2", "w2", "g3"}, default_plan=any(c["plan"] == "" for c, g in n1),
                wg_below_8=any(g["launched"] < 8 for c, g in n1), wg_multiple_of_8=any(g["launched"] % 8 == 0 for c, g in n1),
                wg_neither=any(g["launched"] > 8 and g["launched"] % 8 for c, g in n1))
    assert all(seen.values()), ("n1", [k for k, v in seen.items() if not v])
    w = [(c, f, g) for c, f, g in rows if f in ("t16", "generic")]
    seen = dict(t16_heights={g["TY"] for c, f, g in w if f == "t16" and c["plan"] == ""} >= {4, 8, 12, 16},
                ny17=any(c["mesh"][1] == 17 and g["tiles"] == 2 for c, f, g in w),
                nx17=any(c["mesh"][0] == 17 and g["chunks"] == 2 for c, f, g in w), nx31=any(c["mesh"][0] == 31 and g["chunks"] == 2 for c, f, g in w),
                nx16=any(c["mesh"][0] == 16 for c, f, g in w), two_strips=any(g["strips"] == 2 for c, f, g in w),
                generic_TX_no_power_of_two=any(f == "generic" and c["plan"] == "" and g["TX"] & (g["TX"] - 1) for c, f, g in w),
                one_element=any(c["mesh"] == (2, 2, 2) for c, f, g in w), non_unit_rule=any(c["rule"] == "w2" for c, f, g in w),
                wg_below_8=any(g["launched"] < 8 for c, f, g in w), wg_multiple_of_8=any(g["launched"] % 8 == 0 for c, f, g in w),
                wg_neither=any(g["launched"] > 8 and g["launched"] % 8 for c, f, g in w))
    assert all(seen.values()), ("w", [k for k, v in seen.items() if not v])


def test_masks_sit_on_both_sides_of_every_seam():
    """every mask image of the file: fixed and free nodes on each column, row and plane next to a chunk, tile or strip seam, on the last column,
    row and plane, at the corners; the fp32 images hold 0.5 and both its float32 neighbours"""
    half = np.float32(0.5)
    n = 0
    for case in p.all_cases():
        c = build(case)
        cols, rows, planes = p.seam_lines(c["mesh"], choose(c)[1])
        nx, ny, nz = c["mesh"]
        for m in c["conds"]:
            if m["kind"] == "box":
                continue
            fx = np.stack([p.fixed_nodes(m, c["mesh"], b) for b in range(m["img"].shape[0])])
            n += 1
            if min(c["mesh"]) >= 4:
                assert all(0 < fx[..., x].sum() < fx[..., x].size for x in cols), case
                assert all(0 < fx[:, :, y].sum() < fx[:, :, y].size for y in rows), case
                assert all(0 < fx[:, z].sum() < fx[:, z].size for z in planes), case
            corners = fx[0][np.ix_((0, nz - 1), (0, ny - 1), (0, nx - 1))]
            assert 0 < corners.sum() < 8
            if m["kind"] == "f32" and min(c["mesh"]) >= 4:
                assert all((m["img"] == v).sum() >= 3 for v in (half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)))), case
            if m["kind"] == "u8" and min(c["mesh"]) >= 4:
                assert set(np.unique(m["img"])) == {0, 1, 255}
    assert n > 300


@pytest.mark.parametrize("mesh,rule,fkind", [((5, 4, 3), "g2", "nodal"), ((4, 3, 4), "g3", "gp")], ids=["g2-nodal", "g3-gp"])
def test_reference_is_the_oracle(mesh, rule, fkind):
    """The restatement against oracle.fem_oracle.Oracle with float64 tables: the energy, and the gradient by autograd (alpha = 2 c, beta = 1,
    wscale = jac, out_scale = 1 / (B nel) of torch.mean; a gradient is zero on the Dirichlet nodes).  The oracle's tables are the float32
    roundings of the 3-D products of float64 1-D values, the restatement's the products of float32 1-D values: an entry differs by at most
    2 roundings (half a rounding there, three halves here), a placed product holds two entries, and the eight corner products inside one
    term of a random field cancel to about half their absolute sum -- so node a may differ by 2 x 2 x 2 = 8 x 2^-24 S_a and the energy by
    8 x 2^-24 SE.  Any mistake of the restatement (a swapped axis, a wrong weight, a wrong order of the conditions) is of order 1."""
    import torch
    from test_gpu_switch_invariance import _oracle
    B, ngp = 2, p.NGP[rule]
    nx, ny, nz = mesh
    o = _oracle(dict(nsd=3, domain_sizes=mesh, domain_lengths=tuple((n - 1) * h for n, h in zip(mesh, p.HS)), domain_size=mesh[0], ngp_1d=ngp))
    shape = (nz, ny, nx)
    u, nu = p.rnd((B, *shape), "pin", mesh, "u", lo=-1.0, width=2.0), p.rnd((B, *shape), "pin", mesh, "nu", lo=0.5)
    f = p.rnd((B, *shape), "pin", mesh, "f") if fkind == "nodal" else p.rnd((B, ngp ** 3, nz - 1, ny - 1, nx - 1), "pin", mesh, "f")
    m0, m1 = (p._rng("pin", mesh, k).random((B, *shape)) < 0.25 for k in range(2))
    v0, v1 = p.rnd((B, *shape), "pin", mesh, "v"), 0.3125
    cc, jac = 0.75, 0.25
    nel = (nx - 1) * (ny - 1) * (nz - 1)
    t5 = lambda a: torch.from_numpy(a).double().unsqueeze(1)                 # noqa: E731
    ur = t5(u).requires_grad_(True)
    kw = dict(f=t5(f)) if fkind == "nodal" else dict(f_gp=torch.from_numpy(f).double())
    L = o.energy(ur, t5(nu), dirichlet=[(t5(m0.astype(np.float32)), t5(v0)), (t5(m1.astype(np.float32)), v1)], c=cc, jac=jac, **kw)
    (grad,) = torch.autograd.grad(L, ur)
    E = SE = 0.0
    for b in range(B):
        r = p.poisson3d(u[b], nu[b], f[b], fkind, [m0[b], m1[b]], [v0[b], v1], p.tables(rule), alpha=2 * cc, beta=1.0, c=cc, wscale=jac,
                        out_scale=1.0, scale=True)
        E, SE = E + float(r["energy"]), SE + cc * float(r["SE1"]) + float(r["SE2"])
        d = np.abs(grad[b, 0].numpy() * (B * nel) - r["out"])
        free = ~r["fixed"]
        assert free.any() and r["fixed"].any() and (m0[b] & m1[b]).any()
        print(f"p3-pin {mesh} {rule}: sample {b}: largest |oracle - restatement| / S = {(d[free] / r['S'][free]).max() / U:.3g} x 2^-24")
        assert (d <= 8 * U * r["S"]).all() and (grad[b, 0].numpy()[r["fixed"]] == 0).all()
    d = abs(float(L.detach()) * B * nel - E)
    print(f"p3-pin {mesh} {rule}: energy {float(L.detach()):.12g} against {E / (B * nel):.12g}, |difference| / SE = {d / SE / U:.3g} x 2^-24")
    assert d <= 8 * U * SE


def test_float32_yardsticks():
    """Y per rule and forcing form: finite, of the size of a few float32 roundings per placed product -- and what K = 4 Y therefore is"""
    Y = p.yardsticks()
    assert set(Y) == {(2, "absent"), (2, "nodal"), (2, "gp"), (2, "load"), (3, "absent"), (3, "nodal"), (3, "gp"), (4, "absent"), (4, "nodal"), (4, "gp")}
    for k, (y, case) in sorted(Y.items()):
        print(f"p3-yardstick {k[0]} points, forcing {k[1]}: Y = {y:.3g} = {y / U:.3g} x 2^-24 at {tuple(case)}; K = {MARGIN * y:.3g}")
        assert math.isfinite(y) and y >= U / 2


TEETH = [Case("n1", "w2", "NF", "f32x2", p.MESH_O, 2, "16,16,1,3", "sums", 47), Case("cfz", "g2", "NFL", "u8x2", p.MESH_E, 2, "16,16,2,3", "sums", 47)]


def _mutants(case):
    """(name, `out` of a deliberately wrong float64 evaluation)"""
    c, ref = build(case), reference(case)
    nx, ny, nz = c["mesh"]
    out = []
    if c["fkind"] == "load":
        return [("the load vector scaled by wscale twice", evaluate(c, mutate="load_twice")["out"])]
    assert c["nu"].shape[0] == 1 and all(m["kind"] == "f32" for m in c["conds"])
    both = p.fixed_nodes(c["conds"][0], c["mesh"], 0) & p.fixed_nodes(c["conds"][1], c["mesh"], 0)
    assert both.any()
    out.append(("x and z scales swapped", evaluate(c, mutate="swap_xz")["out"]))
    out.append(("the second condition applied before the first", evaluate(c, mutate="order")["out"]))
    out.append(("the fp32 threshold as >=", evaluate(c, mutate="ge")["out"]))
    out.append(("one Gauss weight of the non-unit rule off by 2^-10", evaluate(c, mutate="weight")["out"]))
    out.append(("a shared nu read as batched", evaluate(c, mutate="nu_batched")["out"]))
    # the top plane's z mass coefficient that of an interior plane: the forcing part of the top plane as if a further layer with the clamped
    # load f(m + 1) = f(m) lay above it
    kw = dict(alpha=0.0, beta=c["beta"], c=0.0, wscale=c["wscale"], out_scale=c["out_scale"])
    m = ref["out"].copy()
    for b in range(c["B"]):
        f = p.pick(c["f"], b)
        fixed = [p.fixed_nodes(x, c["mesh"], b) for x in c["conds"]]
        ext = lambda a: np.concatenate([a, a[-1:]])                   # noqa: E731
        zero = np.zeros_like(f)
        own = p.poisson3d(zero, None, f, "nodal", fixed, [0.0, 0.0], c["tables"], **kw)["out"]
        more = p.poisson3d(ext(zero), None, ext(f), "nodal", [ext(x) for x in fixed], [0.0, 0.0], c["tables"], **kw)["out"]
        m[b, nz - 1] += more[nz - 1] - own[nz - 1]
    out.append(("the top plane's z mass coefficient that of an interior plane", m))
    # a seam column's contribution counted twice at one node: the share of the element left of and below it, from the one-element mesh
    g = choose(c)[1]
    col = g["TX"] - 1
    b = 0
    z, y = next((z, y) for z in range(1, nz - 1) for y in range(1, ny - 1) if not ref["fixed"][b, z, y, col])
    cut = lambda a: a[z - 1:z + 1, y - 1:y + 1, col - 1:col + 1]      # noqa: E731
    fixed = [cut(p.fixed_nodes(x, c["mesh"], b)) for x in c["conds"]]
    share = p.poisson3d(cut(c["u"][b]), cut(p.pick(c["nu"], b)), cut(p.pick(c["f"], b)), "nodal", fixed, [x["value"] for x in c["conds"]], c["tables"],
                        alpha=c["alpha"], beta=c["beta"], c=c["c"], wscale=c["wscale"], out_scale=c["out_scale"])
    m = ref["out"].copy()
    m[b, z, y, col] += share["out"][1, 1, 1]
    assert share["out"][1, 1, 1] != 0
    out.append(("a seam column's contribution counted twice at one node", m))
    return out


@pytest.mark.parametrize("case", TEETH, ids=["n1-w2", "cfz-load"])
def test_comparator_has_teeth(case):
    """The float32 evaluation of the restatement passes (e <= Y by the definition of Y; here on a case of its own data: e <= K); each mutation
    of the float64 restatement lands above K, by the printed factor."""
    c, ref = build(case), reference(case)
    K = K_of(c)
    e32 = node_error(evaluate(c, dtype=np.float32)["out"], ref, c["out_scale"])[0]
    print(f"p3-teeth {case.family}: float32 evaluation: e = {e32:.3g} = {e32 / K:.3g} x K")
    assert e32 <= K
    muts = _mutants(case)
    assert len(muts) == (1 if c["fkind"] == "load" else 7)
    for name, out in muts:
        e = node_error(out, ref, c["out_scale"])[0]
        print(f"p3-teeth {case.family}: {name}: e = {e:.3g} = {e / K:.3g} x K (K = {K:.3g})")
        assert e > K, (name, e, K)
