"""The four operators that share the element march (csrc/elem2d_march.inl) and its host layer (csrc/elem2d_common.h) -- strongform_apply,
fosls_apply, helmholtz_apply, eikonal_apply and its VJP -- against the float64 restatements of their host test files, node by node, on
every template instantiation the host's dispatch can pick (part 1: the full product of the selectors, 597 kernels, at 65 x 6 elements,
B = 2 under PLAN_FSDT "64,4": two chunks with a hand-over column, strips of 4 + 2 element rows with a recomputed layer) and on every
launch seam (part 2: one element, an idle thread, the closing column as a wave's last thread, a second chunk of two thread columns,
one-row strips, three chunks, two- to four-wave workgroups, the default plan past 256 thread columns, tall and narrow, grid.z of 600; each
override also against the default plan, bitwise), with the Dirichlet masks laid on both sides of every seam, on the last row and column
and on the corners, fp32 masks holding 0.5 and its two float32 neighbours.

No tolerance is chosen.  For every free node e = |got - ref64| / S, with S the magnitude field of the float64 restatement
(elem2d_ref.py); where S == 0 the output is exactly 0; Dirichlet nodes are exactly 0 in the strong-form gradient, the FOSLS gradient of
u, the Helmholtz out, eikonal R and its VJP.  A case passes if max e <= K = 4 Y, Y being the largest e the float32 CPU evaluation of
the same restatement reaches over all the cases of the family and mode in this file -- measured against the reference alone, once per
session.  4 is the margin the project gives a fused route over a reference route's own distance to float64.  The sums the kernels add
up per element in fp32 (strong-form and FOSLS sum, Helmholtz energy) are held to n 2^-24 of their magnitude, n the roundings on the
longest path to one element's sum (elem2d_ref.n_roundings); the sums of squares (fp32 per node row of P nodes, then fp64) to
|got - sum ref64^2| <= 2 K sum |ref64| S + (P + 2) 2^-24 sum ref64^2, the norm to the same bound through the square root and one float32
rounding of the stored value.  The CPU tests keep the matrix and the seam list from shrinking and show that the comparator has teeth.

Yardsticks Y (in units of 2^-24) and the largest GPU ratio e / Y per family and mode on the MI355X, with the case that produced it (every
case prints its own; run with -s):
    family and mode   Y     largest e / Y   at (degree, rule, elements, B, plan, form (FK, M, own), output, node)
    strong-form       4.24  0.606           Q2, 3 points, 65 x 6, B = 2, "64,4", (0, 2, no NL, no D2), grad (0, 9, 1)
    FOSLS             6.09  0.516           Q3, 4 points, 65 x 6, B = 2, "64,4", (2, 1, no NUF), g_u (0, 4, 110)
    Helmholtz         6.6   0.412           Q3, 4 points, 65 x 6, B = 2, "64,4", (0, 1, CF 0), out (1, 4, 124)
    eikonal           5.78  0.731           Q3, 4 points, 130 x 9, B = 1, "192,2", (1, 2), R (0, 19, 171)
    eikonal VJP       3.6   0.702           Q1, 2 points, 127 x 9, B = 3, "128,4", (0, 2), vjp (2, 0, 9)
No family comes near the margin of 4: on all 597 instantiations and at every seam the kernels sit closer to float64 than the float32
restatement does at its worst node.  The element sums stay below 0.04 of their bound (strong-form and FOSLS sum 0.012, Helmholtz energy
0.034), the sums of squares below 0.07, every norm lies in its interval, every repeated sample of the 600-sample case is bitwise its
source, no override of the plan changes a bit of an output or moves a sum by 1e-12, no output subset changes a bit, in_den = 0 gives
exact zeros, and at fp32 mask values of 0.5 and its two neighbours every kernel does what the header says (`> 0.5`): neither a kernel
nor the header needed a change.  (Y is recomputed in every session; the float32 CPU arithmetic of another machine may move it by a unit
or so.  The plan mirror shows one thing the header does not say: for meshes of a few thread columns the default rule takes 256
threads, since its 0.0003 T term outweighs the utilisation there.)
"""
import math

import numpy as np
import pytest

import elem2d_ref as q
from elem2d_ref import MARGIN, U, build, evaluate, node_error, reference, yardstick

RATIOS = {}


# ---------------------------------------------------------------------------------------------
# running a case on the GPU
# ---------------------------------------------------------------------------------------------
def _geom(c):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    ny, nx = c["node_shape"]
    return FemGeometry(2, (nx, ny), (q.HX, q.HY), c["P"], c["ngp"], *gauss_rule(c["ngp"]))


def _cu(a):
    from test_gpu_parity import cu
    return cu(a)


def _node(a):
    """(B | 1, ny, nx) -> the (B | 1, 1, ny, nx) device tensor the operators take; constants and None as they are"""
    return _cu(a).unsqueeze(1) if isinstance(a, np.ndarray) else a


def _dev(a):
    return _cu(a) if isinstance(a, np.ndarray) else a


def _one(x):
    return None if x is None else _cu(np.array([x], dtype=np.float32))


class plan_set:
    """PLAN_FSDT for the launches inside, the default plan afterwards"""

    def __init__(self, plan):
        self.plan = plan

    def __enter__(self):
        from diffnet_amd import _lib
        _lib.config_set("PLAN_FSDT", self.plan)

    def __exit__(self, *exc):
        from diffnet_amd import _lib
        _lib.config_set("PLAN_FSDT", "")


def run(c, want=None, packed=False):
    """One launch of the case's operator under the plan in force.  want: the outputs to ask for (None: all).  Returns (outs: a list
    of (B, ny, nx) float32 arrays or None, sums: dict name -> float)."""
    from diffnet_amd import ops
    fam, g = c["family"], _geom(c)
    host = lambda t: None if t is None else t.cpu().numpy()[:, 0]            # noqa: E731
    val = lambda t: float(t.cpu()[0])                                        # noqa: E731
    kw = dict(bc=tuple(_node(m) for m in c["masks"]), bc_values=tuple(_node(v) for v in c["vals"]), f=_node(c["f"]), f_gp=_dev(c["f_gp"]),
              wscale=q.WSCALE)
    w = (lambda n: True) if want is None else (lambda n: n in want)
    sums = {}
    if fam == "strongform":
        grad, s = ops.strongform_apply(g, _node(c["u"]), coef=c["coef"], out_scale=q.OUT_SCALE, in_scale=_one(c["in_scale"]),
                                       want_grad=w("grad"), want_sum=w("sum"), **kw)
        outs = [host(grad)]
        if s is not None:
            sums["sum"] = val(s)
    elif fam == "fosls":
        okw = dict(nu=_node(c["nu"]), weights=q.FO_C["weights"], fs=q.FO_C["fs"], out_scale=q.OUT_SCALE, in_scale=_one(c["in_scale"]),
                   want_sum=w("sum"), **kw)
        if packed:
            fields = _cu(np.stack([c["u"], c["mx"], c["my"]], axis=1))
            grads, s = ops.fosls_apply(g, fields=fields, **okw)
            outs = [grads[:, k].cpu().numpy() for k in range(3)]
        else:
            want3 = tuple(w(n) for n in ("g_u", "g_mx", "g_my"))
            grads, s = ops.fosls_apply(g, _node(c["u"]), _node(c["mx"]), _node(c["my"]), want_grad=want3, **okw)
            outs = [host(t) for t in (grads or (None, None, None))]
        if s is not None:
            sums["sum"] = val(s)
    elif fam == "helmholtz":
        out, en, ss = ops.helmholtz_apply(g, _node(c["u"]), nu=_node(c["nu"]), sigma=_node(c["sigma"]), energy_coef=q.HH_C["ecoef"],
                                          out_coef=q.HH_C["ocoef"], out_scale=q.OUT_SCALE, want_out=w("out"), want_energy=w("energy"),
                                          want_sumsq=w("sumsq"), **kw)
        outs = [host(out)]
        sums.update({n: val(t) for n, t in (("energy", en), ("sumsq", ss)) if t is not None})
    else:
        vjp = fam == "eikonal_vjp"
        out, ss, nrm = ops.eikonal_apply(g, _node(c["u"]), cot=_node(c["cot"]) if vjp else None, in_num=_one(c["in_num"]) if vjp else None,
                                         in_den=_one(c["in_den"]) if vjp else None, want_out=w("R") or w("vjp"), want_sumsq=w("sumsq"),
                                         want_norm=w("norm"), **q.EK_C, **kw)
        outs = [host(out)]
        sums.update({n: val(t) for n, t in (("sumsq", ss), ("norm", nrm)) if t is not None})
    return outs, sums


def judge(spec, outs, sums, K, Y, record=False):
    """Holds every output and sum of one launch to its bound: (the lines of what misses, the lines of every figure).  record: keep the
    family's largest e / Y for the table"""
    c, (ref, rsums), fam = build(spec), reference(spec), spec.family
    B, nref = c["B"], c["nref"]
    weight = np.bincount(np.arange(B) % nref, minlength=nref)
    bad, lines = [], []
    head = f"elem2d-ratio {fam} P={spec.P} ngp={spec.ngp} elements={spec.nelx}x{spec.nely} B={B} plan='{spec.plan}' form={spec.form}"
    assert len(outs) == len(ref)
    for got, o in zip(outs, ref):
        assert got.dtype == np.float32 and got.shape == (B, *c["node_shape"])
        e, at = node_error(got[:nref], o)
        line = f"{head} {o['name']}: e/Y = {e / Y:.3g} at {at} (Y = {Y / U:.3g} x 2^-24)"
        ok = e <= K
        if record and e / Y > RATIOS.get(fam, (0.0, None))[0]:
            RATIOS[fam] = (e / Y, (spec, o["name"], at))
        if B > nref:             # the other samples repeat these inputs: results do not depend on the batch, bit by bit
            same = np.array_equal(got.view(np.uint32), got[np.arange(B) % nref].view(np.uint32))
            line += f" repeats bitwise: {same}"
            ok = ok and same
        lines.append(line)
        if not ok:
            bad.append(line)
    for name, (vals, mags) in rsums.items():
        total, bnd = q.element_sum_bound(spec, vals, mags, weight)
        err = abs(sums[name] - total)
        line = f"{head} {name}: err / bound = {err / bnd if bnd > 0 else float(err != 0):.3g} (n = {q.n_roundings(fam, spec.P, spec.ngp)})"
        lines.append(line)
        if not (err <= bnd and math.isfinite(sums[name])):
            bad.append(line)
    if "sumsq" in sums:
        o = ref[0]
        raw = dict(ref=o["raw"], S=o["S_raw"]) if fam == "helmholtz" else o
        total, bnd = q.sums_bound(raw, K, spec.P, weight)
        s = sums["sumsq"]
        ok = abs(s - total) <= bnd if total > 0 else s == 0.0
        line = f"{head} sumsq: err / bound = {abs(s - total) / bnd if bnd > 0 else float(s != total):.3g}"
        if "norm" in sums:
            lo, hi = math.sqrt(max(total - bnd, 0.0)) * (1 - U), math.sqrt(total + bnd) * (1 + U)
            ok = ok and lo <= sums["norm"] <= hi
            line += f" norm {'in' if lo <= sums['norm'] <= hi else 'OUT OF'} [{lo:.9g}, {hi:.9g}]"
        lines.append(line)
        if not ok:
            bad.append(line)
    return bad, lines


def check(spec, also_default=False):
    """Runs the case under its plan and judges it; every figure is printed before anything is asserted.  also_default: an override case
    runs on the default plan too -- outputs bitwise equal, sums to rtol 1e-12."""
    c = build(spec)
    Y, _ = yardstick(spec.family)
    K = MARGIN * Y
    with plan_set(spec.plan):
        outs, sums = run(c)
    bad, lines = judge(spec, outs, sums, K, Y, record=True)
    print("\n".join(lines))
    if also_default and spec.plan:
        outs0, sums0 = run(c)
        for x, y in zip(outs, outs0):
            if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
                bad.append(f"{spec}: the default plan changes the output")
        for n in sums:
            if not abs(sums[n] - sums0[n]) <= 1e-12 * abs(sums0[n]):
                bad.append(f"{spec}: the default plan moves {n} from {sums[n]!r} to {sums0[n]!r}")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("P,ngp", q.DEGREE_RULES)
@pytest.mark.parametrize("family", q.FAMILIES)
def test_every_instantiation_the_dispatch_can_pick(family, P, ngp):
    """part 1: the full product of the host's selectors for one family, mode, degree and rule (coverage: test_matrix_is_the_full_product)"""
    bad = [b for spec in q.part1_specs(family, P, ngp) for b in check(spec)]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", q.SEAMS, ids=lambda m: "x".join(map(str, m[:3])) + ("-" + m[3].replace(",", "x") if m[3] else ""))
@pytest.mark.parametrize("family", q.FAMILIES)
def test_every_launch_seam(family, mesh):
    """part 2: one seam mesh at three degrees, the widest form with Gauss-point and with nodal forcing; overrides also on the default plan"""
    specs = [s for s in q.part2_specs(family) if (s.nelx, s.nely, s.B, s.plan) == tuple(mesh)]
    assert len(specs) == (3 if family == "eikonal_vjp" else 6)
    bad = [b for spec in specs for b in check(spec, also_default=True)]
    assert not bad, "\n".join(bad)


SUBSETS = dict(strongform=[("grad",), ("sum",)], fosls=[("g_u",), ("g_mx",), ("g_my",), ("sum",)],
               helmholtz=[("out",), ("energy",), ("sumsq",)], eikonal=[("R",), ("sumsq",), ("norm",)], eikonal_vjp=[("vjp",), ("sumsq",), ("norm",)])


@pytest.mark.gpu
@pytest.mark.parametrize("family", q.FAMILIES)
def test_output_subsets_change_no_bit(family):
    """a launch that is asked for one output writes what the all-outputs launch writes, bit by bit; FOSLS: the packed form too"""
    spec = q.part1_specs(family, 2, 3)[-1]
    c = build(spec)
    names = q.NAMES[family]
    with plan_set(spec.plan):
        outs, sums = run(c)
        for want in SUBSETS[family]:
            o1, s1 = run(c, want=want)
            for n, x, y in zip(names, outs, o1):
                assert (y is None) == (n not in want), (want, n)
                if y is not None:
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (want, n)
            assert set(s1) == set(want) & set(sums), (want, s1)
            for n, v in s1.items():
                assert np.float64(v).view(np.uint64) == np.float64(sums[n]).view(np.uint64), (want, n, v, sums[n])
        if family == "fosls":
            o3, s3 = run(c, packed=True)
            for n, x, y in zip(names, outs, o3):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), ("packed", n)
            assert s3["sum"] == sums["sum"]


@pytest.mark.gpu
def test_zz_print_the_largest_ratio_of_every_family():
    """last in the file: the table the module docstring records (empty entries when the tests above were deselected)"""
    for fam in q.FAMILIES:
        Y, where = yardstick(fam)
        r = RATIOS.get(fam)
        print(f"elem2d-family {fam}: Y = {Y / U:.3g} x 2^-24 at {where}; largest GPU e / Y = " + ("not run" if r is None else f"{r[0]:.3g} at {r[1]}"))


# ---------------------------------------------------------------------------------------------
# CPU: the matrix, the seam list, the yardsticks, the comparator's teeth
# ---------------------------------------------------------------------------------------------
def test_matrix_is_the_full_product():
    """the instantiation of every part-1 argument set, derived from the arguments by the host's rules: the full product, each once"""
    counts = dict(strongform=198, fosls=126, helmholtz=189, eikonal=63, eikonal_vjp=21)
    seen = []
    for fam in q.FAMILIES:
        cases = [build(s) for P, ngp in q.DEGREE_RULES for s in q.part1_specs(fam, P, ngp)]
        got = [q.selectors(c) for c in cases]
        want = q.expected_kernels(fam)
        assert len(want) == counts[fam] and len(got) == len(set(got)) == counts[fam] and set(got) == want, (fam, sorted(set(got) ^ want))
        seen += got
        # the runtime sub-forms: each occurs in every family
        batched = lambda xs: {x.shape[0] > 1 for x in xs if isinstance(x, np.ndarray)}          # noqa: E731
        assert batched(m for c in cases for m in c["masks"] if m is not None) == {False, True}            # shared and per-sample masks
        assert batched(v for c in cases for v in c["vals"]) == {False, True}                                # ... value fields
        kinds = {tuple(None if m is None else m.dtype.name for m in c["masks"]) for c in cases}
        assert kinds >= {("float32", "uint8"), ("uint8", None), (None, "float32"), ("float32", "float32"), ("uint8", "uint8"), (None, None)}
        both = [c for c in cases if all(m is not None for m in c["masks"])]
        assert any((q.fixed_nodes(q.pick(c["masks"][0], 0)) & q.fixed_nodes(q.pick(c["masks"][1], 0))).any() for c in both)        # overlap
        f32 = np.concatenate([m.ravel() for c in cases for m in c["masks"] if m is not None and m.dtype == np.float32])
        assert all((f32 == v).sum() >= 100 for v in (q.HALF, q.BELOW, q.ABOVE))                             # the threshold and its neighbours
        if fam != "eikonal_vjp":
            assert batched(c[n] for c in cases for n in ("f", "f_gp")) == {False, True}                     # ... forcings
        if fam in ("strongform", "fosls"):
            assert {c["in_scale"] for c in cases} == {None, q.IN_SCALE}
        if fam == "fosls":
            assert batched(c["nu"] for c in cases) == {False, True}
        if fam == "helmholtz":
            cf2 = {(c["nu"] is not None, isinstance(c["sigma"], np.ndarray)) for c in cases}
            assert cf2 >= {(True, True), (True, False), (False, True)}                                       # nu only, sigma only, both
        if fam == "eikonal_vjp":
            assert {(c["in_num"], c["in_den"]) for c in cases} == {(None, None), (q.IN_NUM, None), (q.IN_NUM, q.IN_DEN), (q.IN_NUM, 0.0)}
            (o,), _ = reference(next(c["spec"] for c in cases if c["in_den"] == 0.0))
            assert not o["S"].any() and not o["ref"].any()           # in_den == 0: S == 0 everywhere, so the comparator asks for exact zeros
        # fixed and free nodes on both sides of every seam, on the last row and column; fixed and free corners
        for c in cases:
            ny, nx = c["node_shape"]
            rows, cols = q.seam_nodes(c["P"], nx, ny, c["B"], c["plan"])
            P = c["P"]
            assert set(cols) >= {63 * P - 1, 63 * P, 63 * P + 1, nx - 1} and set(rows) >= {4 * P - 1, 4 * P, 4 * P + 1, ny - 1}
            free_all = np.ones((ny, nx), bool)
            for m in c["masks"]:
                if m is not None:
                    fx = q.fixed_nodes(m)
                    assert all(0 < fx[:, :, col].sum() < fx[:, :, col].size for col in cols)
                    assert all(0 < fx[:, r].sum() < fx[:, r].size for r in rows)
                    corners = fx[:, [0, 0, -1, -1], [0, -1, 0, -1]]
                    assert 0 < corners.sum() < corners.size
                    free_all &= ~fx.any(axis=0)
            assert all(free_all[:, col].any() for col in cols) and all(free_all[r].any() for r in rows)     # free under both conditions
    assert len(seen) == len(set(seen)) == 198 + 126 + 189 + 84 == 597


def test_seam_list_reaches_every_property():
    """The Python mirror of elem2d_plan on the part-2 list, at every degree the list runs at: the rows of the issue's table, and every
    property the list is there for"""
    for P in (1, 2, 3):
        g = [q.plan(P, P * nelx + 1, P * nely + 1, B, pl) for nelx, nely, B, pl in q.SEAMS]
        assert [(p["T"], p["chunks"], p["R"], p["strips"], p["last"], p["used"]) for p in g] == [
            (256, 1, 1, 1, 1, 2),           # one element: its own column and the closing one (the default rule takes 256 threads for it)
            (64, 1, 3, 1, 3, 63),           # a wave with one idle thread
            (64, 1, 4, 1, 4, 64),           # the closing column is the wave's last thread, one strip
            (128, 1, 4, 2, 1, 65),          # the default plan makes the same mesh one two-wave workgroup
            (64, 2, 4, 2, 1, 2),            # a second chunk of the recomputed and the closing column, last strip of one row
            (64, 2, 1, 7, 1, 64),           # a full second chunk, one-row strips
            (64, 3, 3, 3, 1, 2),            # three chunks, the third of two thread columns, last strip of one row
            (128, 1, 4, 3, 1, 128),         # two waves, the closing column the second wave's last thread
            (192, 1, 2, 5, 1, 131),         # three waves, the last of them with three thread columns
            (256, 1, 2, 1, 2, 256),         # four waves filled to the last thread, R cut down to nely
            (64, 5, 2, 1, 2, 5),            # the default rule past 256 thread columns: five one-wave chunks
            (256, 1, 4, 9, 1, 3),           # tall and narrow: nine default strips, the last of one row
            (256, 1, 2, 1, 2, 3),           # grid.z = 600
            (128, 2, 2, 2, 1, 74)]          # two chunks of two waves
        seen = dict(one_element=g[0]["Q"] == 2, idle_thread=any(p["used"] == p["T"] - 1 and p["chunks"] == 1 for p in g),
                    closing_is_last_thread=any(p["used"] == p["T"] == 64 and p["chunks"] == 1 for p in g),
                    two_column_chunk=any(p["used"] == 2 and p["chunks"] > 1 for p in g),
                    full_later_chunk=any(p["used"] == p["T"] and p["chunks"] > 1 for p in g),
                    three_chunks=any(p["chunks"] == 3 for p in g), one_row_strips=any(p["R"] == 1 and p["strips"] > 1 for p in g),
                    last_strip_of_one_row=any(p["last"] == 1 and p["R"] > 1 for p in g), odd_R=any(p["R"] % 2 == 1 and p["strips"] > 1 for p in g),
                    waves={p["waves"] for p in g} == {1, 2, 3, 4}, chunks_of_several_waves=any(p["waves"] > 1 and p["chunks"] > 1 for p in g),
                    R_cut_to_nely=any(pl == "256,64" and p["R"] == 2 for p, (_, _, _, pl) in zip(g, q.SEAMS)),
                    default_past_256=any(p["Q"] > 256 and not pl for p, (_, _, _, pl) in zip(g, q.SEAMS)),
                    default_strips=any(p["strips"] >= 9 and not pl for p, (_, _, _, pl) in zip(g, q.SEAMS)),
                    grid_z=any(B > 256 for _, _, B, _ in q.SEAMS))
        assert all(seen.values()), (P, [k for k, v in seen.items() if not v])
    # part 1: two chunks with a hand-over column, strips of 4 + 2 element rows
    for P in (1, 2, 3):
        p = q.plan(P, P * q.MESH1[0] + 1, P * q.MESH1[1] + 1, q.MESH1[2], q.PLAN1)
        assert (p["T"], p["chunks"], p["R"], p["strips"], p["last"], p["used"]) == (64, 2, 4, 2, 2, 3)
    # every part-2 case is the widest form of its family: both conditions, one fp32 and one uint8, value fields
    for fam in q.FAMILIES:
        for s in q.part2_specs(fam):
            c = build(s)
            assert [m.dtype.name for m in c["masks"]] == ["float32", "uint8"] and all(isinstance(v, np.ndarray) for v in c["vals"])
            assert q.selectors(c)[3:6] == (True, True, s.form[0])


def test_float32_yardsticks():
    """Y per family and mode: finite, of the size of a few float32 roundings -- and what K = 4 Y therefore is"""
    for fam in q.FAMILIES:
        Y, where = yardstick(fam)
        print(f"elem2d-yardstick {fam}: Y = {Y:.3g} = {Y / U:.3g} x 2^-24 at {where}; K = {MARGIN * Y:.3g}; {len(q.all_specs(fam))} cases")
        assert math.isfinite(Y) and Y >= U / 2        # a float32 evaluation cannot sit closer to float64 than half a rounding of one term


def _mutants(spec):
    """(name, outputs, sums) of deliberately wrong float32 evaluations of one part-1 case: sums as run() returns them"""
    c, (ref, rsums) = build(spec), reference(spec)
    P, fam = spec.P, spec.family
    nely, nelx = c["elem_shape"]
    R = q.plan(P, *c["node_shape"][::-1], c["B"], spec.plan)["R"]

    def sums_of(outs, esums):
        s = {n: float(v.sum()) for n, (v, _) in esums.items()}
        if fam in ("helmholtz", "eikonal", "eikonal_vjp"):
            sq = (outs[0]["raw"] if fam == "helmholtz" else outs[0]["ref"]).astype(np.float64)
            s["sumsq"] = float((sq * sq).sum())
            if fam != "helmholtz":
                s["norm"] = float(np.float32(math.sqrt(s["sumsq"])))
        return s

    def result(**kw):
        outs, esums = evaluate(c, single=True, scale=False, **kw)
        return [o["ref"].copy() for o in outs], sums_of(outs, esums)

    base, base_sums = result()
    out = [("the float32 evaluation itself", base, base_sums)]
    tabs = list(q.tables_f32(P, spec.ngp))
    tabs[1] = tabs[1][:, [1, 0, *range(2, P + 1)]]
    out.append(("two columns of the derivative table swapped", *result(tables=tuple(tabs))))
    # the hand-over: what the elements left of the node column shared between the chunks add to it never arrives
    share, _ = evaluate(q.crop(c, (62, 63), (0, nely)))
    m = [x.copy() for x in base]
    for x, s in zip(m, share):
        x[:, :, 63 * P] -= s["ref"][:, :, -1].astype(np.float32)
    out.append(("the hand-over column's contribution dropped", m, base_sums))
    m = [x.copy() for x in base]
    for x, b in zip(m, base):
        x[:, R * P + 1] = b[:, R * P]
    out.append(("the strip's first node row stored one row further up", m, base_sums))
    out.append(("condition 1 wins where both hold", *result(first_wins=True)))
    out.append(("`>= 0.5` for `> 0.5`", *result(ge=True)))
    b, j, i = np.argwhere(ref[0]["fixed"] & (ref[0]["S"] == 0))[0]
    jf, i_f = next((jj, ii) for jj in range(c["node_shape"][0]) for ii in range(c["node_shape"][1]) if not ref[0]["fixed"][b, jj, ii] and base[0][b, jj, ii] != 0)
    m = [x.copy() for x in base]
    m[0][b, j, i] = base[0][b, jf, i_f]
    out.append(("a Dirichlet node not zeroed", m, base_sums))
    # the recomputed layer under the second strip counted in both strips
    twice = dict(base_sums)
    _, layer = evaluate(q.crop(c, (0, nelx), (R - 1, R)), scale=False)
    for n, (v, _) in layer.items():
        twice[n] = base_sums[n] + float(v.sum())
    if "sumsq" in twice:
        row = (reference(spec)[0][0]["raw"] if fam == "helmholtz" else base[0]).astype(np.float64)[:, R * P]
        twice["sumsq"] = base_sums["sumsq"] + float((row * row).sum())
        if "norm" in twice:
            twice["norm"] = float(np.float32(math.sqrt(twice["sumsq"])))
    out.append(("a seam layer counted twice in the sums", base, twice))
    return out


@pytest.mark.parametrize("family", q.FAMILIES)
def test_comparator_has_teeth(family):
    """Mutations of the float32 evaluation of the widest case of the part-1 matrix at Q2: each lands above 10 K at some node, or outside
    the bound of a sum; the float32 evaluation itself passes"""
    spec = next(s for P, ngp in q.DEGREE_RULES[3:] for s in reversed(q.part1_specs(family, P, ngp))
                if s.form[1] == 2 and all(m is not None and (m.dtype == np.uint8 or (m == q.HALF).any()) for m in build(s)["masks"])
                and any(m.dtype == np.float32 for m in build(s)["masks"]))
    print(f"elem2d-teeth {family}: {spec}")
    Y, _ = yardstick(family)
    K = MARGIN * Y
    muts = _mutants(spec)
    assert len(muts) == 8
    for k, (name, outs, sums) in enumerate(muts):
        bad, lines = judge(spec, [np.asarray(x, dtype=np.float32) for x in outs], sums, K, Y)
        e = max(node_error(x, o)[0] for x, o in zip(outs, reference(spec)[0]))
        print(f"elem2d-teeth {family}: {name}: e = {e / K:.3g} x K; sums out of bound: {sum('err / bound' in b for b in bad)}")
        if k == 0:
            assert not bad and e <= Y, (name, bad)
        else:
            assert e > 10 * K or any("err / bound" in b for b in bad), (name, e / K, lines)
