"""The four fused Q1 residual operators that share the 62-column wave layout and flow2d_plan (csrc/flow2d_common.h) -- stokes_apply,
ns_apply, transport_apply and poisson_coef_grad (2-D; its plain 3-D kernel too) -- against the float64 restatements of their host test
files, node by node, on every template instantiation the host's dispatch can pick (part 1: the full product of the selectors at 64 x 10
nodes, B = 2, two chunks and two or three strips) and on every launch seam (part 2: a full chunk, a chunk of one owner column, odd and
even rows per strip, a last strip of one row, idle waves, strips limited by the batch; coef-grad also under PLAN2D overrides of R).

No tolerance is chosen.  For every free node e = |got - ref64| / S, with S the sum of |w_g t| over the placed terms that make up the
node's value in the float64 restatement (q1_residual_ref.py); where S == 0 the output is exactly 0; Dirichlet nodes hold the float32
boundary value (forward), exactly 0 (VJP, Stokes transpose); coef-grad has no Dirichlet rows (include/diffnet_hip.h).  A case passes if
max e <= K = 4 Y, Y being the largest e the float32 CPU evaluation of the same restatement reaches over all the cases of the family in
this file -- measured against the reference alone, once per session.  4 is the margin the project gives a fused route over a reference
route's own distance to float64 (test_strongform_fused_matches_composed).  The sums of squares (fp32 per lane over a strip of R rows,
then fp64) are held to |got - sum ref64^2| <= 2 K sum |ref64| S + (R + 2) 2^-24 sum ref64^2, the norms to the same bound through the
square root and one float32 rounding of the stored value.  The CPU tests keep the matrix and the seam list from shrinking (the selector
mirror against the full product, the plan mirror against the library's workspace sizes) and show that the comparator has teeth.

Yardsticks Y (in units of 2^-24) and the largest GPU ratio e / Y per family on the MI355X, with the case that produced it (every case
prints its own; run with -s):
    family          Y     largest e / Y   at (rule, mesh, B, form, output, node)
    Stokes          7.88  0.944           3 points, 62 x 9, B = 2, (sel 1, FGP), R3 (1, 8, 0): the first column of the last row, last strip
    Stokes^T        17.6  0.483           3 points, 64 x 10, B = 2, (sel 1, FGP given, dropped), out 3 (0, 9, 0)
    NS              7.93  1.34            2 points, 64 x 10, B = 2, (sel 0, FGP), R3 (0, 0, 0): a corner node, one element
    NS VJP          13.6  0.498           4 points, 64 x 10, B = 2, (sel 1, no FGP), out 1 (1, 9, 31)
    transport       9.9   0.595           4 points, 64 x 17, B = 3, (no NU, no REACT, sel 0, no FGP), (0, 16, 0)
    transport VJP   7.39  0.952           2 points, 125 x 26, B = 2, (NU, REACT, sel 2, FGP given), (1, 0, 6)
    coef-grad 2-D   14.3  0.46            3 points, 64 x 10, B = 2, (no v, nu and f, fp32 masks with a field), g_nu (0, 0, 33)
    coef-grad 3-D   24.8  0.416           4 points, 65 x 4 x 3, B = 2, (v, u8 masks with a field), g_nu (0, 0, 0, 0)
No family comes near the margin of 4: the kernels sit as close to float64 as the float32 restatement does, boundary nodes with few terms
being the worst in both.  The sums of squares stay below 0.1 of their bound, every repeated sample of the 600-sample case is bitwise its
source, the PLAN2D overrides change no bit, and at fp32 mask values of 0.5 and its neighbours every kernel does what its header says
(`>= 0.5` in flow2d_fixed and transport.hip, `> 0.5` in cg_set): neither a kernel nor the header needed a change.  (Y is recomputed in
every session; the float32 CPU arithmetic of another machine may move it by a unit or so.)
"""
import ctypes as C
import math

import numpy as np
import pytest

import q1_residual_ref as q
from q1_residual_ref import MARGIN, U, Spec, build, evaluate, node_error, reference, yardstick

RATIOS = {}


# ---------------------------------------------------------------------------------------------
# running a case on the GPU
# ---------------------------------------------------------------------------------------------
def _geom(c):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    mesh = c["mesh"]
    return FemGeometry(len(mesh), mesh, (q.HX, q.HY, q.HZ)[:len(mesh)], 1, c["ngp"], *gauss_rule(c["ngp"]))


def _cu(a):
    from test_gpu_parity import cu
    return cu(a)


def _node(a):
    """(B | 1, *node_shape) -> the (B | 1, 1, *node_shape) device tensor the operators take; constants as they are"""
    return _cu(a).unsqueeze(1) if isinstance(a, np.ndarray) else a


def _dev(a):
    return _cu(a) if isinstance(a, np.ndarray) else a


def run(c):
    """One launch of the case's operator.  Returns (outs: list of (B, *node_shape) float32 arrays, sums | None, norms | None)."""
    from diffnet_amd import ops
    fam, g = c["family"], _geom(c)
    host = lambda t: t.cpu().numpy()[:, 0]                                   # noqa: E731
    masks = [_node(m) for m in c["masks"]]
    vals = tuple(_node(v) for v in c["vals"])
    if fam in ("stokes", "stokes_t", "ns", "ns_vjp"):
        flds = [_node(f) for f in c["fields"]]
        f = tuple(_dev(x) for x in c["f"])
        if fam in ("stokes", "stokes_t"):
            k = q.STOKES_C
            outs, sums, norms = ops.stokes_apply(g, *flds, tuple(masks), vals, k["visco"], k["pspg"], f, k["J"], want_norms=True,
                                                 transpose=fam == "stokes_t")
        else:
            k = q.NS_C
            cot = [_node(t) for t in c["cot"]] if fam == "ns_vjp" else None
            outs, sums, norms = ops.ns_apply(g, *flds, tuple(masks), vals, k["visco"], f, k["J"], k["tau_h"], k["cinv"], cot=cot, want_norms=True)
        return [host(o) for o in outs], sums.cpu().numpy(), norms.cpu().numpy()
    if fam in ("transport", "transport_vjp"):
        k = q.TRANSPORT_C
        out, sums, norm = ops.transport_apply(g, _node(c["u"]), _node(c["nu"]) if c["nu"] is not None else None, tuple(masks), vals, c["first"],
                                              _dev(c["f"]), k["adv"], k["kappa"], k["tau"], c["react"], k["J"],
                                              cot=_node(c["cot"]) if fam == "transport_vjp" else None, want_norm=True)
        return [host(out)], sums.cpu().numpy(), norm.cpu().numpy()
    k = q.COEF_C
    sc = None if c["in_scale"] is None else _cu(np.array([c["in_scale"]], dtype=np.float32))
    g_nu, g_f = ops.poisson_coef_grad(g, _node(c["u"]), None if c["v"] is None else _node(c["v"]), list(zip(masks, vals)), k["a_nu"], k["a_f"],
                                      k["wscale"], c["want"], sc)
    assert (g_nu is None) == ("nu" not in c["want"]) and (g_f is None) == ("f" not in c["want"])
    return [host(t) for t in (g_nu, g_f) if t is not None], None, None


def check(spec):
    """Runs the case and holds every output, sum and norm to the bound; every figure is printed before anything is asserted."""
    c, ref, fam = build(spec), reference(spec), spec.family
    Y, _ = yardstick(fam)
    K = MARGIN * Y
    outs, sums, norms = run(c)
    B, nref = c["B"], c["nref"]
    bad = []
    assert len(outs) == len(ref)
    for k, (got, o) in enumerate(zip(outs, ref)):
        assert got.dtype == np.float32 and got.shape == (B, *c["node_shape"])
        e, at = node_error(got[:nref], o)
        prev = RATIOS.get(fam, (0.0, None))
        if e / Y > prev[0]:
            RATIOS[fam] = (e / Y, (spec, o["name"], at))
        line = f"q1-ratio {fam} ngp={spec.ngp} mesh={spec.mesh} B={B} form={spec.form} {o['name']}: e/Y = {e / Y:.3g} at {at} (Y = {Y / U:.3g} x 2^-24)"
        if not e <= K:
            bad.append(line)
        if B > nref:             # the other samples repeat these inputs: the kernels promise results independent of the batch, bit by bit
            same = np.array_equal(got.view(np.uint32), got[np.arange(B) % nref].view(np.uint32))
            line += f" repeats bitwise: {same}"
            if not same:
                bad.append(line)
        if sums is not None:
            w = np.bincount(np.arange(B) % nref, minlength=nref)
            R = q.plan(*spec.mesh, B, q.MIN_ROWS[q.OPERATOR[fam]])["R"]
            total, bnd = q.sums_bound(o, K, R, w)
            lo, hi = math.sqrt(max(total - bnd, 0.0)) * (1 - U), math.sqrt(total + bnd) * (1 + U)
            s, n = float(sums[k]), float(norms[k])
            ok = (abs(s - total) <= bnd and lo <= n <= hi) if total > 0 else (s == 0.0 and n == 0.0)
            line += f" sumsq err/bound = {abs(s - total) / bnd if bnd > 0 else float(s != total):.3g} norm {'in' if lo <= n <= hi else 'OUT OF'} [{lo:.9g}, {hi:.9g}]"
            if not ok:
                bad.append(line)
        print(line)
    return bad


FLOW2D = [f for f in q.FAMILIES if f != "coef3d"]


@pytest.mark.gpu
@pytest.mark.parametrize("ngp", [2, 3, 4])
@pytest.mark.parametrize("family", q.FAMILIES)
def test_every_instantiation_the_dispatch_can_pick(family, ngp):
    """part 1: the full product of the host's selectors for one operator, mode and rule (coverage: test_matrix_is_the_full_product)"""
    bad = [b for spec in q.part1_specs(family, ngp) for b in check(spec)]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", q.SEAMS, ids=lambda m: "x".join(map(str, m)))
@pytest.mark.parametrize("family", FLOW2D)
def test_every_launch_seam(family, mesh):
    """part 2: one seam mesh, three forms (everything, nothing, one between)"""
    specs = [s for s in q.part2_specs(family) if (*s.mesh, s.B) == tuple(mesh)]
    assert len(specs) == 3
    bad = [b for spec in specs for b in check(spec)]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", [(63, 25, 1), (64, 17, 3), (125, 26, 2)], ids=lambda m: "x".join(map(str, m)))
def test_coef_grad_plan_overrides_change_no_bit(mesh):
    """coef_grad_plan (poisson_coef_grad.hip:387-401): R = 1, 3 and ny through PLAN2D; the results are those of the default plan, bitwise"""
    from diffnet_amd import _lib
    specs = [s for s in q.part2_specs("coef2d") if (*s.mesh, s.B) == tuple(mesh)]
    base = [run(build(s))[0] for s in specs]
    try:
        for R in (1, 3, mesh[1]):
            _lib.config_set("PLAN2D", f"64,2,{R}")
            for s, b in zip(specs, base):
                got = run(build(s))[0]
                for x, y in zip(got, b):
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (s, R)
    finally:
        _lib.config_set("PLAN2D", "")


@pytest.mark.gpu
@pytest.mark.parametrize("family", q.FAMILIES)
def test_fp32_masks_at_the_threshold_follow_the_header(family):
    """fp32 mask values of exactly 0.5 and of its two float32 neighbours: a Dirichlet node from 0.5 on in dn_stokes_args, dn_ns_args and
    dn_transport_args (`>= 0.5`), only above it in dn_dirichlet (`> 0.5`: dn_coef_grad_args) -- the reference takes the header's side"""
    (spec,) = q.threshold_specs(family)
    c = build(spec)
    img = np.concatenate([m.ravel() for m in c["masks"] if m is not None])
    half = np.float32(0.5)
    assert all((img == v).sum() >= 3 for v in (half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1))))
    bad = check(spec)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_zz_print_the_largest_ratio_of_every_family():
    """last in the file: the table the module docstring records (empty entries when the tests above were deselected)"""
    for fam in q.FAMILIES:
        Y, where = yardstick(fam)
        r = RATIOS.get(fam)
        print(f"q1-family {fam}: Y = {Y / U:.3g} x 2^-24 at {where}; largest GPU e / Y = " + ("not run" if r is None else f"{r[0]:.3g} at {r[1]}"))


# ---------------------------------------------------------------------------------------------
# CPU: the matrix, the seam list, the yardsticks, the comparator's teeth
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", q.FAMILIES)
def test_matrix_is_the_full_product(family):
    """the selector tuple of every part-1 argument set, derived from the arguments by the host's rules, covers the full product"""
    nargs = dict(stokes=6, stokes_t=6, ns=6, ns_vjp=6, transport=24, transport_vjp=24, coef2d=30, coef3d=10)[family]
    nkern = dict(stokes=6, stokes_t=2, ns=6, ns_vjp=6, transport=24, transport_vjp=10, coef2d=28, coef3d=10)[family]
    for ngp in (2, 3, 4):
        cases = [build(s) for s in q.part1_specs(family, ngp)]
        assert len(cases) == nargs and len({s.form for s in q.part1_specs(family, ngp)}) == nargs
        got = {q.selectors(c) for c in cases}
        want = q.expected_kernels(family, ngp)
        assert len(want) == nkern and got == want, (family, ngp, sorted(got ^ want))
    cases = [build(s) for ngp in (2, 3, 4) for s in q.part1_specs(family, ngp)]
    batched = lambda xs: {x.shape[0] > 1 for x in xs if isinstance(x, np.ndarray)}          # noqa: E731
    assert batched(m for c in cases for m in c["masks"] if m is not None) == {False, True}            # shared and per-sample masks
    assert batched(v for c in cases for v in c["vals"]) == {False, True}                                # ... value fields
    if family in ("stokes", "ns", "ns_vjp", "transport"):
        assert batched(f for c in cases for f in (c["f"] if isinstance(c["f"], list) else [c["f"]])) == {False, True}      # ... forcings
    if family in ("ns", "ns_vjp", "stokes", "stokes_t"):
        kinds = {tuple(None if m is None else m.dtype.name for m in c["masks"]) for c in cases}
        assert ("float32", "uint8", None) in kinds                               # three fields, three mask kinds
        assert any(sum(isinstance(f, np.ndarray) for f in c["f"]) == 1 for c in cases)        # only one of f_gp[0], f_gp[1] a tensor
    if family.startswith("transport"):
        both = [c for c in cases if all(m is not None for m in c["masks"])]
        assert {c["first"] for c in both} == {False, True}
        assert any((q.fixed_nodes(q.pick(c["masks"][0], 0)) & q.fixed_nodes(q.pick(c["masks"][1], 0))).any() for c in both)        # overlapping conditions
    # nodes fixed and free on both sides of the chunk seam and of every strip seam
    if family != "coef3d":
        for c in cases:
            for m in c["masks"]:
                if m is not None:
                    fx = q.fixed_nodes(m, coef=family == "coef2d")
                    assert all(0 < fx[:, :, col].sum() < fx[:, :, col].size for col in (61, 62, 63))
                    assert all(0 < fx[:, r].sum() < fx[:, r].size for r in q.seam_rows(c["node_shape"][0], c["B"], c["node_shape"][1]))


def test_seam_list_reaches_every_seam():
    """The Python mirror of flow2d_plan on the part-2 list: every seam property is reached under both shortest strips, and the mirror is
    the library's plan wherever the library shows it without a GPU (the reduction workspaces hold k doubles per workgroup and sample)."""
    from diffnet_amd import _lib
    from test_stokes_host import stokes_mesh
    h = _lib.lib()
    for mr in (4, 8):
        plans = [q.plan(nx, ny, B, mr) for nx, ny, B in q.SEAMS]
        seen = dict(full_chunk=any(p["last_owners"] == q.OWNERS for p in plans),
                    full_chunks_2=any(p["last_owners"] == q.OWNERS and p["chunks"] == 2 for p in plans),
                    one_owner_chunk=any(p["last_owners"] == 1 and p["chunks"] > 1 for p in plans),
                    three_chunks=any(p["chunks"] == 3 for p in plans),
                    odd_R=any(p["R"] % 2 == 1 and p["strips"] >= 2 for p in plans),
                    even_R=any(p["R"] % 2 == 0 and p["strips"] >= 2 for p in plans),
                    last_strip_of_one_row=any(p["last"] == 1 and p["strips"] >= 2 for p in plans),
                    idle_waves=any(p["idle"] > 0 for p in plans),
                    one_strip=any(p["strips"] == 1 for p in plans),
                    batch_limited=any(p["batch_limited"] for p in plans))
        assert all(seen.values()), (mr, [k for k, v in seen.items() if not v])
    # the rows of the issue's table
    assert [(p["chunks"], p["strips"], p["R"], p["last"], p["idle"]) for p in (q.plan(nx, ny, B, 8) for nx, ny, B in q.SEAMS)] == \
        [(1, 1, 2, 2, 0), (1, 2, 5, 4, 0), (1, 2, 5, 4, 0), (2, 4, 7, 4, 0), (2, 3, 6, 5, 2), (2, 2, 8, 7, 0), (3, 4, 7, 5, 0), (1, 8, 8, 1, 0),
         (1, 7, 10, 4, 1)]
    assert [(p["strips"], p["R"], p["last"], p["idle"]) for p in (q.plan(nx, ny, B, 4) for nx, ny, B in q.SEAMS[1:7])] == \
        [(3, 3, 3, 0), (3, 3, 3, 0), (7, 4, 1, 2), (5, 4, 1, 2), (4, 4, 3, 0), (7, 4, 2, 3)]
    for nx, ny, B in q.SEAMS + [q.MESH1]:
        for op, fn in (("stokes", h.dn_stokes_workspace_bytes), ("ns", h.dn_ns_workspace_bytes), ("transport", h.dn_transport_workspace_bytes)):
            m = stokes_mesh(n=nx, ny=ny, B=B)
            gx = q.plan(nx, ny, B, q.MIN_ROWS[op])["gx"]
            assert fn(C.byref(m)) == q.WS_HEADER + q.WS_DOUBLES[op] * 8 * gx * B, (op, nx, ny, B, gx)


def test_float32_yardsticks():
    """Y per family: finite, of the size of a few float32 roundings per placed term -- and what K = 4 Y therefore is"""
    for fam in q.FAMILIES:
        Y, where = yardstick(fam)
        print(f"q1-yardstick {fam}: Y = {Y:.3g} = {Y / U:.3g} x 2^-24 at {where}; K = {MARGIN * Y:.3g}; {len(q.all_specs(fam))} cases")
        assert math.isfinite(Y) and Y > 0
        assert Y >= U / 2          # a float32 evaluation cannot sit closer to float64 than half a rounding of one term


def _mutants(spec):
    """(name, outputs of a deliberately wrong float64 evaluation) of one case at 64 x 10, B = 2"""
    c, ref = build(spec), reference(spec)
    ny, nx = c["node_shape"]
    out = []
    vals = lambda r: [o["ref"].copy() for o in r]                             # noqa: E731
    # 1. the element left of column 62 contributes nothing to that column in one row: its share is the residual of the one-element mesh
    b, fixed = 0, ref[0]["fixed"]
    row = next(r for r in range(1, ny - 1) if not fixed[b, r, 62] and ref[0]["S"][b, r, 62] > 0)
    sub = {k: v for k, v in c.items()}
    cut = lambda a, e=0: a[(slice(b, b + 1) if a.shape[0] > 1 else slice(0, 1)), ..., row:row + 2 - e, 61:63 - e] if isinstance(a, np.ndarray) else a      # noqa: E731
    for k in ("fields", "cot", "masks", "vals", "u", "nu"):
        if k in sub and sub[k] is not None:
            sub[k] = [cut(a) for a in sub[k]] if isinstance(sub[k], list) else cut(sub[k])
    sub["f"] = [cut(a, 1) for a in c["f"]] if isinstance(c["f"], list) else cut(c["f"], 1)
    sub.update(mesh=(2, 2), node_shape=(2, 2), B=1, nref=1)
    share = evaluate(sub)
    m = vals(ref)
    m[0][b, row, 62] -= share[0]["ref"][0, 0, 1]
    out.append(("one element's share of a column-62 node dropped", m))
    # 2. the forcing of Gauss point g + 1 read for point g
    roll = lambda a: np.roll(a, -1, axis=1) if isinstance(a, np.ndarray) else a        # noqa: E731
    out.append(("forcing of point g + 1 read for point g", vals(evaluate(dict(c, f=[roll(a) for a in c["f"]] if isinstance(c["f"], list) else roll(c["f"]))))))
    # 3. the x and y derivative scales exchanged
    out.append(("x and y derivative scales exchanged", vals(evaluate(c, swap_scales=True))))
    # 4. a per-sample mask read from sample 0
    first = lambda a: np.repeat(a[:1], a.shape[0], axis=0) if isinstance(a, np.ndarray) else a       # noqa: E731
    assert any(isinstance(a, np.ndarray) and a.shape[0] > 1 for a in c["masks"])
    out.append(("per-sample masks read from sample 0", vals(evaluate(dict(c, masks=[first(a) for a in c["masks"]])))))
    # 5. condition 1 wins where both hold (transport: NS has one condition per field)
    if spec.family == "transport":
        m0, m1 = c["masks"]
        assert (q.fixed_nodes(m0) & q.fixed_nodes(m1)).any()
        out.append(("condition 1 wins where both hold", vals(evaluate(dict(c, masks=[m0, np.where(q.fixed_nodes(m0), 0, m1).astype(m1.dtype)])))))
    # 6. the first row of the second strip stored one row further down
    R = q.plan(nx, ny, c["B"], 8)["R"]
    m = vals(ref)
    for k in range(len(m)):
        m[k][:, R + 1] = ref[k]["ref"][:, R]
    out.append(("a strip's first row moved to the row below it", m))
    return out


@pytest.mark.parametrize("spec", [Spec("ns", 3, q.MESH1[:2], q.MESH1[2], (2, True), 5), Spec("transport", 3, q.MESH1[:2], q.MESH1[2], (True, True, 2, True), 23)],
                         ids=["ns", "transport"])
def test_comparator_has_teeth(spec):
    """Each mutation of the float64 reference of a masked, forced case lands above K, by the printed factor.  (The float32 evaluation of
    every case of the family sits at or below Y = K / 4: that is how Y is defined, so it is said here, not asserted.)"""
    assert spec in q.part1_specs(spec.family, spec.ngp)
    ref = reference(spec)
    Y, _ = yardstick(spec.family)
    K = MARGIN * Y
    muts = _mutants(spec)
    assert len(muts) == (6 if spec.family == "transport" else 5)
    for name, outs in muts:
        e = max(node_error(x, o)[0] for x, o in zip(outs, ref))
        print(f"q1-teeth {spec.family}: {name}: e = {e:.3g} = {e / K:.3g} x K (K = {K:.3g})")
        assert e > K, (name, e, K)
