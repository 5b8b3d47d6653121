"""The fused 3-D eikonal residual and its VJP (csrc/eikonal3d.hip, built for 3 and 4 points through eikonal3d_g3.hip and eikonal3d_g4.hip;
dn_eikonal3d_apply / ops.eikonal3d_apply) against the float64 restatement of the header's formula (eikonal3d_ref.py), node by node, on every
template instantiation the host can pick (part 1: the full product of 3 rules by 12 forms, 36 kernels, at 17 x 9 x 7 elements, B = 2, under
"PLAN3D" "8,8,1,3": 3 chunks x 2 tiles x 3 strips x 2 samples = 36 one-wave workgroups, strips that march 3, 4 and 2 layers) and on every
launch seam (part 2: one element, a closing column owned by the tile's last thread, a chunk whose only owner has no element, the default
plan's row seam, strips of one plane, odd and even layer counts, a last strip of one own layer, one- and four-wave workgroups, wide and
narrow ones, grids that are and are not a multiple of 8, B = 600) on one PF forward kernel, one non-PF forward kernel and one VJP kernel per
rule.  Every case runs under its override AND under the default plan: `out` must be bitwise the same, the sums bitwise equal run to run and
within 1e-12 across plans.

No tolerance is chosen.  For every free node e = |got - ref64| / S, S the restatement on absolute values (eikonal3d_ref.py); where S == 0 the
output is exactly 0; Dirichlet nodes are exactly 0.  A case passes if max e <= K = 4 Y, Y being the largest e the float32 CPU evaluation of
the same restatement reaches over all the cases of this file with the same mode (R, VJP) -- measured against the reference alone, once per
session.  sumsq is held to eikonal3d_ref.sumsq_bound (derived there from emit_plane and dn_reduce.h: one float32 rounding of the square, then
float64), the norm to the same interval through the square root plus one float32 rounding.

Yardsticks Y in units of 2^-24 (recomputed in every session; the float32 CPU arithmetic of another machine may move them by a unit or so):
    R     2.53   (4 points, constant f, masks with constants)
    VJP   2.96   (4 points, masks with value fields)
What the MI355X gave: the largest e / Y per mode and rule (the bound is 4), with the case (every case prints its own; run with -s):
    mode   rule       e / Y   at
    R      2 points   0.475   70 x 3 x 5 elements, B = 2, f at Gauss points, value fields, default plan (the "64,2,1,2" override: the same bits)
    R      3 points   0.568   part 1, constant f, value fields
    R      4 points   0.722   condition 2 alone, 9 x 6 x 5 elements, B = 2, constant f, constants
    VJP    2 points   0.319   9 x 5 x 7 elements, B = 2, value fields ("16,4,1,3": the same bits)
    VJP    3 points   0.316   part 1, masks with constants
    VJP    4 points   0.553   5 x 40 x 9 elements, value fields ("2,32,1,4": the same bits)
The largest |sumsq - ref| over its bound is 0.019 (16 x 3 x 1 elements, B = 2, 4 points, masks with constants); every norm lies inside its
interval.  No kernel comes near the margin of 4: each is closer to float64 than the float32 restatement (the sum-factorised differences
a1 - a0 of neighbouring values are exact where the restatement's eight-term sums are not).  Every override is bitwise the default plan on all
36 kernels and all seam meshes, the sums are bitwise run to run and equal to 1e-12 across plans, every repeat of the B = 600 launches is
bitwise its source, an absent condition is never read from u (u above 0.5 on free nodes), fp32 masks at 0.5 and its lower neighbour are
free and at the upper neighbour fixed, uint8 masks of 2 and 255 fix like 1, in_den == 0 gives an exactly zero VJP: no kernel and no line of
the header needed a change.
"""
import ctypes as C
import math

import numpy as np
import pytest

import eikonal3d_ref as e3
from eikonal3d_ref import K_of, build, geometry, node_error, reference
from poisson3d_ref import HS
from q1_residual_ref import MARGIN, U

RATIOS = {}


def label(case):
    form = ("VJP" if case.vjp else "R f=" + ("const", "nodal", "gp")[case.fk]) + " cond=" + case.cond
    return f"{case.name} {case.ngp} points {form} {'x'.join(map(str, case.nel))} B={case.B} plan={case.plan or 'default'} i={case.i}"


# ---------------------------------------------------------------------------------------------
# running a case on the GPU
# ---------------------------------------------------------------------------------------------
def _geom(c):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(c["ngp"])
    return FemGeometry(3, c["nodes"], HS, 1, c["ngp"], gx, gw)


def device_args(c, times=1, in_den=None):
    """the arguments of ops.eikonal3d_apply as device tensors; times: every per-sample array repeated that often along the batch (sample b of
    the launch is sample b % B of the case)"""
    import torch
    from test_gpu_parity import cu, dev

    def rep(a):
        return np.tile(a, (times,) + (1,) * (a.ndim - 1)) if times > 1 and a.shape[0] > 1 else a

    t5 = lambda a: cu(rep(a)).unsqueeze(1)                       # noqa: E731
    one = lambda x: None if x is None else torch.tensor([x], dtype=torch.float32, device=dev())       # noqa: E731
    d = dict(geom=_geom(c), u=cu(np.tile(c["u"], (times, 1, 1, 1))).unsqueeze(1), tau=c["tau"], sq=c["sq"], wscale=c["wscale"])
    d["bc"] = tuple(None if m is None else t5(m["img"]) for m in c["conds"])
    d["vals"] = tuple(0.0 if m is None else (t5(m["value"]) if isinstance(m["value"], np.ndarray) else m["value"]) for m in c["conds"])
    d["f"] = t5(c["f"]) if c["fkind"] == "nodal" else None
    d["f_gp"] = cu(rep(c["f"])) if c["fkind"] == "gp" else c["fconst"]
    d["cot"] = None if c["cot"] is None else cu(np.tile(c["cot"], (times, 1, 1, 1))).unsqueeze(1)
    num = 1.5 if (c["in_num"] is None and in_den is not None) else c["in_num"]            # in_den needs in_num
    d["in_num"], d["in_den"] = one(num), one(c["in_den"] if in_den is None else in_den)
    return d


def launch(d, plan="", want_out=True, want_sums=True):
    """one launch under "PLAN3D" = plan: (out (B, nz, ny, nx) | None, sumsq | None, norm (float32) | None)"""
    import torch
    from diffnet_amd import _lib, ops
    _lib.config_set("PLAN3D", plan)
    ops.call_cache_clear()
    try:
        out, ss, nrm = ops.eikonal3d_apply(d["geom"], d["u"], d["bc"], d["vals"], d["f"], d["f_gp"], tau=d["tau"], sq=d["sq"], wscale=d["wscale"],
                                           cot=d["cot"], in_num=d["in_num"], in_den=d["in_den"], want_out=want_out, want_sumsq=want_sums,
                                           want_norm=want_sums)
        torch.cuda.synchronize()
    finally:
        _lib.config_set("PLAN3D", "")
        ops.call_cache_clear()
    return (None if out is None else out.cpu().numpy()[:, 0], None if ss is None else float(ss.cpu()[0]),
            None if nrm is None else nrm.cpu().numpy().reshape(()).copy())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def judge(case, ref, got, what, times=1):
    """every figure of one launch against its bound; returns the lines that failed (all are printed first).  times: the launch holds the
    case's samples that often (the node comparison takes the first repeat)"""
    out, sumsq, norm = got
    Y = e3.yardsticks()[e3.mode(case)][0]
    K = MARGIN * Y
    bad = []
    assert out.dtype == np.float32
    e, at = node_error(out[:case.B], ref)
    line = f"ek3-ratio [{label(case)}] {what}: e/Y = {e / Y:.3g} at {at} (Y = {Y / U:.3g} x 2^-24)"
    key = (e3.mode(case), case.ngp)
    if e / Y > RATIOS.get(key, (0.0, None))[0]:
        RATIOS[key] = (e / Y, f"{label(case)} {what}")
    if not e <= K:
        bad.append(line)
    if sumsq is not None:
        want, bound = times * ref["sumsq"], e3.sumsq_bound(ref, K, times)
        lo, hi = e3.norm_interval(ref, K, times)
        rs = abs(sumsq - want) / bound if bound > 0 else float(sumsq != want)
        ok = lo <= float(norm) <= hi and norm.dtype == np.float32
        line += f" sumsq err/bound = {rs:.3g} norm {'inside' if ok else 'OUTSIDE'} [{lo:.9g}, {hi:.9g}]"
        if not (rs <= 1 and ok and math.isfinite(sumsq)):
            bad.append(line)
    print(line)
    return bad


def check(case):
    """the case under the default plan and under its override: both judged, `out` bitwise equal, the sums bitwise equal run to run and equal
    to 1e-12 across plans"""
    c, ref = build(case), reference(case)
    d = device_args(c)
    base = launch(d)
    bad = judge(case, ref, base, "default plan")
    plan = case.plan
    got = launch(d, plan) if plan else base
    again = launch(d, plan)
    if plan:
        bad += judge(case, ref, got, "override")
        assert same_bits(got[0], base[0]), f"{label(case)}: `out` under the override is not bitwise the default plan's"
        assert abs(got[1] - base[1]) <= 1e-12 * abs(base[1]), (label(case), got[1], base[1])
    assert same_bits(again[0], got[0]) and again[1] == got[1] and float(again[2]) == float(got[2]), f"{label(case)}: not bitwise run to run"
    return bad


PART1 = e3.part1_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(PART1)), ids=lambda k: f"g{PART1[k].ngp}-{PART1[k].cond}-" + ("vjp" if PART1[k].vjp else f"f{PART1[k].fk}"))
def test_every_instantiation(k):
    """part 1: one of the 36 kernels (coverage: test_matrix_is_the_full_product)"""
    bad = check(PART1[k])
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(e3.SEAMS)), ids=lambda k: "x".join(map(str, e3.SEAMS[k][0])) + f"-B{e3.SEAMS[k][1]}-{e3.SEAMS[k][2] or 'default'}")
def test_every_launch_seam(k):
    """part 2: one seam mesh on the nine seam kernels (what it reaches: test_seam_list_reaches_every_property)"""
    bad = [b for case in e3.part2_cases()[9 * k:9 * k + 9] for b in check(case)]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(9), ids=lambda k: f"g{e3.batch_cases()[k].ngp}-" + ("pf", "nopf", "vjp")[k % 3])
def test_large_batch(k):
    """B = 600 on 2 x 2 x 2 elements, the samples cycling through three distinct ones: the first three against the reference, every repeat
    bitwise its source, sumsq 200 times the three's sum within the bound of the sums"""
    case = e3.batch_cases()[k]
    c, ref = build(case), reference(case)
    times = e3.BATCH_B // e3.BATCH_BASE
    got = launch(device_args(c, times=times))
    assert got[0].shape == (e3.BATCH_B, *c["shape"])
    rep = got[0].reshape(times, e3.BATCH_BASE, *c["shape"])
    assert all(same_bits(rep[t], rep[0]) for t in range(times)), "a repeated sample is not bitwise its source"
    bad = judge(case, ref, got, "B = 600", times=times)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(e3.only_cases())), ids=lambda k: f"{e3.only_cases()[k].name[4:]}-g{e3.only_cases()[k].ngp}-{k}")
def test_one_condition_alone(k):
    """condition 1 alone and condition 2 alone, u above 0.5 on free nodes: the dummy read of u is no mask"""
    bad = check(e3.only_cases()[k])
    assert not bad, "\n".join(bad)


SUBSET = [PART1[3], PART1[12 + 8], PART1[24 + 11]]          # one form per schedule: PF forward, non-PF forward, VJP (2, 3, 4 points)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SUBSET, ids=["pf", "nopf", "vjp"])
def test_output_subsets_change_no_bit(case):
    """want_out=False leaves sumsq and norm bitwise unchanged; asking for no sums leaves out bitwise unchanged"""
    d = device_args(build(case))
    for plan in (case.plan, ""):
        whole = launch(d, plan)
        sums_only = launch(d, plan, want_out=False)
        out_only = launch(d, plan, want_sums=False)
        assert sums_only[0] is None and sums_only[1] == whole[1] and float(sums_only[2]) == float(whole[2]), (label(case), plan)
        assert out_only[1] is None and out_only[2] is None and same_bits(out_only[0], whole[0]), (label(case), plan)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [PART1[9], PART1[12 + 10], PART1[24 + 11]], ids=["g2-none", "g3-const", "g4-field"])
def test_vjp_with_a_zero_norm_is_exactly_zero(case):
    """in_den == 0 (the norm's VJP at ||R|| = 0, torch's convention): every entry of the VJP is exactly zero, sums included"""
    d = device_args(build(case), in_den=0.0)
    for plan in (case.plan, ""):
        out, sumsq, norm = launch(d, plan)
        assert np.all(out == 0.0) and sumsq == 0.0 and float(norm) == 0.0, (label(case), plan)


@pytest.mark.gpu
@pytest.mark.parametrize("case", e3.threshold_cases(), ids=["pf", "nopf", "vjp"])
def test_fp32_mask_threshold(case):
    """fp32 mask values of 0.5 and of its lower float32 neighbour leave the node free, the upper neighbour fixes it (`> 0.5`): judged by the
    reference, and directly -- the first two nodes carry a value, the third is exactly 0"""
    c, ref = build(case), reference(case)
    free0, free1, fixed = e3.EDGE_NODES
    assert not ref["fixed"][(0, *free0)] and not ref["fixed"][(0, *free1)] and ref["fixed"][(0, *fixed)]
    assert ref["out"][(0, *free0)] != 0 and ref["out"][(0, *free1)] != 0
    bad = check(case)
    out = launch(device_args(c), case.plan, want_sums=False)[0]
    assert out[(0, *free0)] != 0 and out[(0, *free1)] != 0 and out[(0, *fixed)] == 0
    assert not bad, "\n".join(bad)


BOTH = [PART1[5], PART1[12 + 10], PART1[24 + 6]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BOTH, ids=["g2-nopf", "g3-vjp", "g4-pf"])
def test_condition_two_wins_where_both_hold(case):
    """against the reference, not only between two GPU runs: the launch is within K of the restatement and NOT within K of the restatement with
    the two conditions applied in the other order; the Dirichlet nodes are exactly 0"""
    c, ref = build(case), reference(case)
    out = launch(device_args(c), case.plan, want_sums=False)[0]
    K = K_of(case)
    wrong = dict(ref, out=e3.evaluate(c, mutate="order")[0])
    e, e_wrong = node_error(out, ref)[0], node_error(out, wrong)[0]
    print(f"ek3-order [{label(case)}]: e = {e / K:.3g} K against the header's order, {e_wrong / K:.3g} K against the other")
    assert e <= K < e_wrong
    assert ref["fixed"].any() and np.all(out[ref["fixed"]] == 0.0)


@pytest.mark.gpu
def test_zz_print_the_largest_ratio_of_every_mode_and_rule():
    """last in the file: the table the module docstring records (empty entries when the tests above were deselected)"""
    Y = e3.yardsticks()
    for m in ("R", "VJP"):
        print(f"ek3-yardstick {m}: Y = {Y[m][0] / U:.3g} x 2^-24 at [{label(Y[m][1])}]")
        for ngp in e3.RULES:
            r = RATIOS.get((m, ngp))
            print(f"ek3-largest {m} {ngp} points: " + ("not run" if r is None else f"e / Y = {r[0]:.3g} at [{r[1]}]"))


# ---------------------------------------------------------------------------------------------
# CPU: the matrix, the mirrors, the seam list, the masks, the reference, the yardstick, the comparator's teeth
# ---------------------------------------------------------------------------------------------
def test_matrix_is_the_full_product():
    """36 distinct (NGP, MASK, BCF, FK, VJP) tuples by the dispatch mirror -- the 3 x 12 the launch functions instantiate --, both load
    schedules, and across the matrix shared and per-sample tensors for value fields, forcing and masks, every mask format, one condition
    alone and both, both values of tau, no in_num / in_num / in_num with in_den"""
    built = [build(x) for x in PART1]
    got = {e3.dispatch(c) for c in built}
    forms = [(False, False, fk, False) for fk in (0, 1, 2)] + [(True, False, fk, False) for fk in (0, 1, 2)] + \
        [(True, True, fk, False) for fk in (0, 1, 2)] + [(False, False, 0, True), (True, False, 0, True), (True, True, 0, True)]
    assert len(PART1) == 36 and len(got) == 36 and got == {(ngp, *f) for ngp in (2, 3, 4) for f in forms}
    for ngp in e3.RULES:
        assert sorted(e3.is_pf(s) for s in got if s[0] == ngp) == [False] * 7 + [True] * 5
    g = geometry(built[0]["nodes"], 2, e3.PLAN1)
    assert all(c["B"] == 2 and c["nel"] == (17, 9, 7) and c["plan"] == e3.PLAN1 for c in built)
    assert (g["chunks"], g["tiles"], g["strips"], g["grid"], g["waves"], g["layers"]) == (3, 2, 3, 36, 1, [3, 4, 2]) and g["grid"] % 8
    batched = lambda xs: {x.shape[0] > 1 for x in xs}          # noqa: E731
    conds = [m for c in built for m in c["conds"] if m is not None]
    assert batched(m["img"] for m in conds) == {False, True}
    assert batched(m["value"] for m in conds if isinstance(m["value"], np.ndarray)) == {False, True}
    assert batched(c["f"] for c in built if c["fkind"] == "nodal") == {False, True} and batched(c["f"] for c in built if c["fkind"] == "gp") == {False, True}
    assert {m["img"].dtype for m in conds} == {np.dtype(np.float32), np.dtype(np.uint8), np.dtype(bool)}
    assert {tuple(m is not None for m in c["conds"]) for c in built} == {(False, False), (True, False), (False, True), (True, True)}
    for vjp in (False, True):
        assert {c["tau"] for c in built if (c["cot"] is not None) == vjp} == {0.0, 0.25}
    assert {(c["in_num"], c["in_den"]) for c in built if c["cot"] is not None} == {(None, None), (1.5, None), (1.5, 0.75)}
    assert all(c["sq"] != 1.0 + c["tau"] and c["wscale"] != 1.0 for c in built) and len(set(HS)) == 3
    # every cotangent is non-zero on Dirichlet nodes
    for x, c in zip(PART1, built):
        if c["cot"] is not None and x.cond != "none":
            assert np.all(c["cot"][reference(x)["fixed"]] != 0)


def test_seam_list_reaches_every_property():
    """by the plan mirror alone: what the part-2 meshes reach"""
    rows = [(nel, B, plan, tuple(n + 1 for n in nel), geometry(tuple(n + 1 for n in nel), B, plan)) for nel, B, plan in e3.SEAMS]
    rows.append((e3.BATCH_NEL, e3.BATCH_B, "", (3, 3, 3), geometry((3, 3, 3), e3.BATCH_B)))
    own = lambda r: e3.column_owners(r[3], r[4])               # noqa: E731
    seen = dict(
        one_element=any(nel == (1, 1, 1) and B == 1 and g["layers"] == [1] for nel, B, plan, nodes, g in rows),
        column_seam=any(g["chunks"] > 1 for *_, g in rows), row_seam=any(g["tiles"] > 1 for *_, g in rows), layer_seam=any(g["strips"] > 1 for *_, g in rows),
        default_row_seam=any(plan == "" and nel[1] == 16 and (g["TY"], g["tiles"]) == (12, 2) for nel, B, plan, nodes, g in rows),
        closing_column_owned_by_the_last_thread=any(plan == "" and g["chunks"] == 1 and own(r)[0][-1] == (g["TX"] - 1, False) for r in rows for plan, g in [(r[2], r[4])]),
        a_chunk_whose_only_owner_has_no_element=any(plan == "" and [o for o in own(r)[-1]] == [(nodes[0] - 1, False)] for r in rows for plan, nodes in [(r[2], r[3])]),
        strips_of_one_plane=any(g["R"] == 1 and g["layers"] == [1, 2, 2] for *_, g in rows),
        marches_1=any(1 in g["layers"] for *_, g in rows), marches_2=any(2 in g["layers"] for *_, g in rows),
        marches_3=any(3 in g["layers"][1:] for *_, g in rows), marches_4=any(4 in g["layers"][1:] for *_, g in rows),
        R2_later_strips_march_3=any(g["R"] == 2 and g["strips"] > 2 and set(g["layers"][1:-1]) == {3} for *_, g in rows),
        R3_later_strips_march_4=any(g["R"] == 3 and g["strips"] > 2 and set(g["layers"][1:-1]) == {4} for *_, g in rows),
        top_plane_by_a_strip_of_one_own_layer=any(g["strips"] > 1 and g["R"] > 1 and g["own"][-1] == 1 for *_, g in rows),
        nelz_1_and_2_on_the_default_plan={nel[2] for nel, B, plan, nodes, g in rows if plan == ""} >= {1, 2},
        waves_1=any(g["waves"] == 1 for *_, g in rows), waves_4=any(g["waves"] == 4 for *_, g in rows),
        shapes={(g["TX"], g["TY"]) for *_, g in rows} >= {(8, 8), (32, 2), (16, 16), (128, 2), (64, 2), (2, 32)},
        narrow_every_column_a_seam=any(g["TX"] == 2 and nel[0] == 5 and g["chunks"] == 5 and all(len(o) == 1 for o in own(r)[1:])
                                       for r in rows for nel, g in [(r[0], r[4])]),
        grid_multiple_of_8=any(g["grid"] % 8 == 0 for *_, g in rows), grid_no_multiple_of_8=any(g["grid"] > 8 and g["grid"] % 8 for *_, g in rows),
        large_batch=any(B == 600 for _, B, *_ in rows),
        default_plan_past_one_tile_in_all_directions=any(plan == "" and nel == (17, 16, 5) and B == 2 and min(g["chunks"], g["tiles"], g["strips"]) > 1
                                                         for nel, B, plan, nodes, g in rows))
    assert all(seen.values()), [k for k, v in seen.items() if not v]
    # every seam mesh runs one PF forward kernel, one non-PF forward kernel and one VJP kernel per rule
    cases = e3.part2_cases()
    assert len(cases) == 9 * len(e3.SEAMS)
    for k in range(len(e3.SEAMS)):
        sel = [e3.dispatch(build(x)) for x in cases[9 * k:9 * k + 9]]
        assert sorted((s[0], s[4], e3.is_pf(s)) for s in sel) == sorted((ngp, v, pf) for ngp in (2, 3, 4) for v, pf in ((False, True), (False, False), (True, False)))


def _mesh_struct(c, B):
    return _geom(c).mesh_struct(B)


def test_every_plan_is_accepted_and_the_mirror_is_the_library_plan():
    """Every "PLAN3D" string of the file passes the kernel's acceptance conditions and differs from the default plan (an override the host
    silently ignored would test nothing); and the library, asked without a device for its workspace size under every plan of the file
    (4160 + 8 bytes per workgroup), has the mirror's number of workgroups.  The default rule is also test_eikonal3d_host.default_plan's."""
    from diffnet_amd import _lib
    from test_eikonal3d_host import default_plan
    h = _lib.lib()
    seen = set()
    try:
        for case in e3.all_cases():
            c = build(case)
            B = e3.BATCH_B if case.name == "batch" else case.B
            if (case.nel, B, case.plan, case.ngp) in seen:
                continue
            seen.add((case.nel, B, case.plan, case.ngp))
            m = _mesh_struct(c, B)
            g0 = geometry(c["nodes"], B)
            assert (g0["TX"], g0["TY"], g0["R"]) == default_plan(m)
            for plan in {case.plan, ""}:
                g = geometry(c["nodes"], B, plan)
                if plan:
                    assert e3.plan_accepted(plan), plan
                    assert (g["TX"], g["TY"], g["R"]) != (g0["TX"], g0["TY"], g0["R"]), (case, "the override is the default plan")
                assert h.dn_config_set(b"PLAN3D", plan.encode()) == 0
                assert h.dn_eikonal3d_workspace_bytes(C.byref(m)) == 4160 + 8 * g["grid"], (case, plan, g)
    finally:
        h.dn_config_set(b"PLAN3D", b"")
    for bad in ("8,4,1,4", "16,32,1,4", "16,16,1,0", "1,64,1,2", "16,16,1", ""):
        assert not e3.plan_accepted(bad)


def test_masks_keep_no_failure_hidden():
    """every case of the file: the Dirichlet nodes are at most 40 % of a sample; every seam column, row and plane of the plans in force (the
    case's and the default) has fixed and free nodes on it and beside it; u exceeds 0.5 somewhere, and in the cases with one condition alone
    on a quarter of the free nodes at least; where both conditions exist they overlap with different values; fp32 images hold 0.5 and both its
    neighbours, uint8 images 1, 2 and 255"""
    n_only = {"first": 0, "second": 0}
    for case in e3.all_cases():
        c, fx = build(case), reference(case)["fixed"]
        assert (c["u"] > 0.5).any()
        conds = [m for m in c["conds"] if m is not None]
        if not conds:
            assert not fx.any()
            continue
        assert fx.reshape(case.B, -1).mean(axis=1).max() <= 0.40, case
        assert fx[:, 0, 0, 0].all()
        if case.name != "threshold":
            both_kinds = lambda a: a.size < 8 or 0 < a.sum() < a.size          # noqa: E731
            for plan in (case.plan, ""):
                cols, rows, planes = e3.seam_lines(c["nodes"], geometry(c["nodes"], case.B, plan))
                for b in range(case.B):
                    assert all(both_kinds(fx[b, :, :, x]) for x in cols), (case, plan)
                    assert all(both_kinds(fx[b, :, y]) for y in rows), (case, plan)
                    assert all(both_kinds(fx[b, z]) for z in planes), (case, plan)
        if len(conds) == 1:
            free = ~fx
            assert (c["u"][free] > 0.5).mean() >= 0.25, case
            if case.name.startswith("only"):
                n_only[case.name[4:]] += 1
        elif case.name != "threshold":
            both = np.broadcast_to(e3.fixed_nodes(conds[0]["img"]), fx.shape) & np.broadcast_to(e3.fixed_nodes(conds[1]["img"]), fx.shape)
            v0, v1 = (np.broadcast_to(np.asarray(m["value"], np.float32), fx.shape) for m in conds)
            assert both.any() and (v0[both] != v1[both]).all(), case
        for m in conds:
            if m["img"].dtype == np.float32 and case.name == "part1":
                assert all((m["img"] == v).sum() >= 2 for v in e3.EDGE), case
            if m["img"].dtype == np.uint8 and m["img"].size >= 64 * m["img"].shape[0] and case.name != "threshold":
                assert set(np.unique(m["img"])) == {0, 1, 2, 255}, case
    assert n_only["first"] >= 3 and n_only["second"] >= 3
    assert {e3.dispatch(build(x))[1:] for x in e3.only_cases()} == {(True, False, 0, False), (True, True, 2, False), (True, True, 0, True)}


@pytest.mark.parametrize("ngp", [2, 3, 4])
def test_reference_is_the_host_restatement(ngp):
    """the vectorised restatement against eikonal3d_t64 and eikonal3d_pullback_np of test_eikonal3d_host.py, both on float64 tables, to float64
    rounding: unequal spacings, wscale != 1, sq != 1 + tau, tau 0 and 0.25, constant / nodal / Gauss-point forcing, two overlapping conditions
    with value fields; and S bounds |R| node by node"""
    import torch
    from test_eikonal3d_host import _tables, eikonal3d_pullback_np, eikonal3d_t64
    nx, ny, nz = 5, 4, 6
    shp = (nz, ny, nx)
    rs = np.random.default_rng(50 + ngp)
    m1, m2 = rs.random(shp) < 0.2, rs.random(shp) < 0.2
    m1[0, 0, 0] = m2[0, 0, 0] = True
    v1, v2 = 2 * rs.random(shp) - 1, 2 * rs.random(shp) - 1
    u0, cot = 2 * rs.random(shp) - 1, 2 * rs.random(shp) - 1
    Bt, Dt, gw = _tables(ngp, *HS)[:3]
    fn, fg = rs.random(shp), rs.random((ngp ** 3, nz - 1, ny - 1, nx - 1))
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)          # noqa: E731
    f32 = lambda a: np.asarray(a, np.float32)                      # noqa: E731   (the restatement reads float32 inputs)
    u0, cot, v1, v2, fn, fg = (f32(a).astype(np.float64) for a in (u0, cot, v1, v2, fn, fg))
    for tau in (0.0, 0.25):
        for masks, vals in (((None, None), (0.0, 0.0)), ((m1, m2), (v1, v2)), ((None, m2), (0.0, -0.25))):
            fixed = [m for m in masks if m is not None]
            vv = [v for m, v in zip(masks, vals) if m is not None]
            for f, fkind in ((0.75, None), (fn, "nodal"), (fg, "gp")):
                want = eikonal3d_t64(t(u0), *HS, ngp, tau, 1.375, f if fkind is None else t(f), 0.25, masks,
                                     tuple(t(v) if isinstance(v, np.ndarray) else v for v in vals)).numpy()
                got, fx = e3.eikonal3d(f32(u0), fixed, [f32(v) for v in vv], f if fkind is None else f32(f), fkind, None, 1.0, (Bt, Dt, gw), tau, 1.375, 0.25)
                S = e3.eikonal3d(f32(u0), fixed, [f32(v) for v in vv], f if fkind is None else f32(f), fkind, None, 1.0, (Bt, Dt, gw), tau, 1.375, 0.25,
                                 magnitude=True)[0]
                assert np.abs(want).max() > 1e-3 and np.all(np.abs(got - want) <= 2.0 ** -43 * S)
                assert np.all(np.abs(got) <= S * (1 + 1e-12)) and np.all(S[fx] == 0) and np.all(S[~fx] > 0)
            want = eikonal3d_pullback_np(u0, 2.0 * cot, *HS, ngp, tau, 1.375, 0.25, masks, vals)
            got, fx = e3.eikonal3d(f32(u0), fixed, [f32(v) for v in vv], None, None, f32(cot), 2.0, (Bt, Dt, gw), tau, 1.375, 0.25)
            S = e3.eikonal3d(f32(u0), fixed, [f32(v) for v in vv], None, None, f32(cot), 2.0, (Bt, Dt, gw), tau, 1.375, 0.25, magnitude=True)[0]
            assert np.abs(want).max() > 1e-3 and np.all(np.abs(got - want) <= 2.0 ** -43 * S)
            assert np.all(np.abs(got) <= S * (1 + 1e-12)) and np.all(got[fx] == 0)


def test_float32_yardsticks():
    """Y per mode: finite, non-zero, of the size of a few float32 roundings -- and what K = 4 Y therefore is"""
    Y = e3.yardsticks()
    assert set(Y) == {"R", "VJP"}
    for m, (y, case) in sorted(Y.items()):
        print(f"ek3-yardstick {m}: Y = {y:.3g} = {y / U:.3g} x 2^-24 at [{label(case)}]; K = {MARGIN * y:.3g}")
        assert math.isfinite(y) and U / 2 <= y <= 64 * U


def test_the_sum_bound_is_inside_the_stated_one():
    """the derived bound of sumsq (eikonal3d_ref.sumsq_bound) is nowhere wider than 2 K sum |r| S + K^2 sum S^2 + 2^-23 sum r^2"""
    for case in e3.all_cases():
        ref, K = reference(case), K_of(case)
        for times in (1, 200):
            stated = times * (2 * K * ref["abs_S"] + K * K * ref["S2"] + 2.0 ** -23 * ref["sumsq"])
            assert 0 < e3.sumsq_bound(ref, K, times) <= stated, case
            lo, hi = e3.norm_interval(ref, K, times)
            assert lo < math.sqrt(times * ref["sumsq"]) < hi


# (mutation, the part-1 case it is applied to): indices into PART1 are 12 x rule + form (eikonal3d_ref.FORMS)
TEETH = [("dz", "the z-derivative of one z-point dropped", PART1[12 + 1]),
         ("seam", "the recomputed layer under a strip's first plane left out at one seam", PART1[3]),
         ("gp_order", "f_gp with i and k swapped", PART1[12 + 2]),
         ("order", "the second condition applied before the first", PART1[5]),
         ("ge", "the fp32 threshold as >=", PART1[5]),
         ("sq2", "sq2 taken as sq", PART1[9]),
         ("cot", "the cotangent not zeroed on the Dirichlet nodes", PART1[10]),
         ("weight", "one 1-D weight of the 4-point rule replaced by its neighbour", PART1[24])]


@pytest.mark.parametrize("mutate,what,case", TEETH, ids=[t[0] for t in TEETH])
def test_comparator_has_teeth(mutate, what, case):
    """The float32 evaluation of the restatement passes (e <= Y by the definition of Y); the mutation of the float64 restatement, judged as if
    it were the GPU's output, lands above K at some node, by the printed factor."""
    c, ref, K = build(case), reference(case), K_of(case)
    e32 = node_error(e3.evaluate(c, dtype=np.float32)[0], ref)[0]
    assert e32 <= K / MARGIN
    if mutate == "seam":
        g = geometry(c["nodes"], case.B, case.plan)
        assert g["strips"] > 1
        out = e3.seam_layer_left_out(c, ref, g["R"])
    else:
        out = e3.evaluate(c, mutate=mutate)[0]
    e, at = node_error(out, ref)
    print(f"ek3-teeth {what} [{label(case)}]: e = {e:.3g} = {e / K:.3g} x K at {at} (float32 evaluation: {e32 / K:.3g} x K)")
    assert e > K, (what, e, K)
