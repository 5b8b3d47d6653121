"""The batched CG solve on the GPU (dn_poisson_diag, dn_poisson_cg, diffnet_amd/solve.py) against the float64 reference of
tests/solve_ref.py.

Shapes: the smallest at which the kernels can go wrong -- 9^2 (81 nodes: one workgroup, quads and a one-node tail), 17^2 B = 3 (289: odd,
samples 1 and 2 start off 16-byte alignment), 33 x 20 (ny != nx), 65^2 B = 2 (4225: five workgroups a sample plus a tail), 9^3 B = 2,
17 x 9 x 12.  The vector phases cut a sample into chunks of 1024 nodes and every sample arrives at counters of its own, so the
DN_NSHARD = 64 workgroup seam of arrive_last lies at 65 536 nodes a sample (above 130^2): no dense solve reaches it, and the phase test
runs it on flat arrays of 70 001 nodes (69 workgroups a sample).

Bounds.  The diagonal: a sum of non-negative terms, so a relative bound n 2^-24 with n counted in `DIAG_ROUNDINGS`.  The phases: dot
products are float64 sums of exact products of float32 values (rtol 1e-12 covers any order of n <= 1e5 additions), alpha / beta one
float32 rounding of a float64 quotient, x, r, p a count of roundings times 2^-24 times the magnitude of the terms.  The whole solve:
float32 CG is not reproducible across summation orders but its attainable accuracy is, so every comparison with the dense float64
solution is bounded by 4 x the same quantity of solve_ref's float32 run of that sample, which the test computes.
Largest observed ratios (MI355X, profiles/poisson_solve.txt; the tests print them): solution error 1.20, residual gap 1.27, gradients 1.82
of the float32 reference's, against the margin of 4."""
import itertools

import numpy as np
import pytest
import torch

import solve_ref as sr
from test_solve_host import geometry

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MARGIN = 4.0
# dn_poisson_diag per node: <= 64 terms nu_b t, each t from three float32 tables (3 roundings), two or three products and two adds (<= 7),
# the product with nu_b (1); <= 64 additions; wscale (1); the reciprocal (1).  All terms are >= 0 for nu >= 0: the bound is relative.
DIAG_ROUNDINGS = 3 + 7 + 1 + 64 + 2
# colour probing through dn_poisson_apply: per node <= 8 elements x 64 points of non-negative terms, each a handful of roundings; counted
# generously as twice the diagonal's own
PROBE_ROUNDINGS = 2 * DIAG_ROUNDINGS


def dev():
    return torch.device("cuda")


def cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev())


def box_image(shp):
    box = np.zeros(shp, bool)
    for ax in range(len(shp)):
        idx = [slice(None)] * len(shp)
        idx[ax] = 0; box[tuple(idx)] = True
        idx[ax] = -1; box[tuple(idx)] = True
    return box


class Case:
    """One batch: numpy float64 / bool inputs per sample for the reference, torch inputs for the solver."""

    def __init__(self, name, sizes, B, ngp, seed):
        self.name, self.sizes, self.B, self.ngp = name, sizes, B, ngp
        self.geom = geometry(sizes, ngp=ngp)
        self.shp = tuple(self.geom.node_shape)
        self.rng = np.random.default_rng(seed)
        self.jac = float(np.prod([0.5 * h for h in self.geom.hs]))
        self.nu = self.f = self.f_gp = self.u0 = None          # numpy (B | 1, *shp) or None
        self.cond = []                                        # [(mask (B | 1, *shp) bool, value float or (B | 1, *shp) array, form)]
        self._ref = {}

    # per-sample views for the reference
    def pick(self, a, b):
        return None if a is None else a[b if a.shape[0] > 1 else 0]

    def conditions(self, b, homogeneous=False):
        return [(self.pick(m, b), 0.0 if homogeneous else (v if np.ndim(v) == 0 else self.pick(v, b))) for m, v, _ in self.cond]

    def system(self, b):
        """(K, b) of sample b; a stiffness matrix shared by the batch is built once."""
        kk = ("K", b if (self.nu is not None and self.nu.shape[0] > 1) else 0)
        if kk not in self._ref:
            self._ref[kk] = sr.dense_stiffness(self.geom, self.pick(self.nu, b), self.jac)
        if ("b", b) not in self._ref:
            self._ref[("b", b)] = sr.dense_load(self.geom, self.pick(self.f, b), self.pick(self.f_gp, b), self.jac)
        return self._ref[kk], self._ref[("b", b)]

    def reference(self, b, tol=1e-6, unit=False):
        """(u64, x32, info32, err32) of sample b: the dense solution, solve_ref's float32 run and its error, computed once."""
        key = ("ref", b, tol, unit)
        if key not in self._ref:
            K, rhs = self.system(b)
            cond = self.conditions(b)
            x0 = self.pick(self.u0, b)
            u64 = sr.dense_solve(K, rhs, cond, x0)
            fx = sr.fixed_nodes(len(rhs), cond)
            x32, info = sr.cg_restated(K, rhs, cond, x0, dinv=sr.dense_dinv(K, fx, unit), tol=tol, maxiter=20 * max(self.shp), dtype=np.float32)
            scale = max(np.max(np.abs(u64)), 1e-300)
            self._ref[key] = (u64, x32, info, np.max(np.abs(x32 - u64)) / scale)
        return self._ref[key]

    # torch side
    def torch_inputs(self, samples=None):
        """kwargs of poisson_solve / PoissonSolver for the whole batch or for the listed samples."""
        from diffnet_amd import ops
        sel = (lambda a: a) if samples is None else (lambda a: a if a.shape[0] == 1 else a[samples])
        t = lambda a: None if a is None else cu(sel(a))[:, None] if a.ndim == len(self.shp) + 1 else cu(sel(a))
        dl = []
        for m, v, form in self.cond:
            mm = sel(m)[:, None]
            if form == "box":
                mask = ops.BoxFaces("all")
            elif form == "packed":
                mask = ops.PackedMask.pack(cu(mm, torch.uint8))
            else:
                mask = cu(mm, torch.uint8 if form == "u8" else torch.float32)
            dl.append(ops.Dirichlet(mask, float(v) if np.ndim(v) == 0 else cu(sel(v))[:, None]))
        kw = dict(nu=t(self.nu), f=t(self.f), dirichlet=dl, u0=t(self.u0), jac=self.jac,
                  batch=self.B if samples is None else len(samples))
        if self.f_gp is not None:
            kw["f_gp"] = cu(sel(self.f_gp))
        return kw


def make_cases():
    cases = {}
    # A: 9^2 B = 1 -- random nu, nodal f, box faces (no image) + an interior fp32 blob with a value field, random u0
    c = Case("9x9", (9, 9), 1, 2, 101)
    c.nu = c.rng.uniform(0.5, 1.5, (1, *c.shp)); c.f = 10 * c.rng.standard_normal((1, *c.shp)); c.u0 = c.rng.standard_normal((1, *c.shp))
    blob = np.zeros((1, *c.shp), bool); blob[0, 3:5, 4:6] = True
    c.cond = [(box_image(c.shp)[None], 0.0, "box"), (blob, c.rng.standard_normal((1, *c.shp)), "f32")]
    cases[c.name] = c
    # B: 17^2 B = 3 -- sample 1 contrast 100, sample 2 a zero patch of nu (f zero there); per-sample uint8 masks, constant 0.5; 3-point rule
    c = Case("17x17", (17, 17), 3, 3, 102)
    c.nu = c.rng.uniform(0.5, 1.5, (3, *c.shp))
    c.nu[1] = np.where(c.rng.random(c.shp) < 0.5, 0.01, 1.0)
    c.nu[2, 5:11, 6:12] = 0.0
    c.f = 10 * c.rng.standard_normal((3, *c.shp)); c.f[2, 5:11, 6:12] = 0.0
    m = np.repeat(box_image(c.shp)[None], 3, 0)
    for b in range(3):
        m[b, 2 + b, 3:6] = True
    c.cond = [(m, 0.5, "u8")]
    cases[c.name] = c
    # C: 33 x 20 B = 2 -- shared nu and f, a shared fp32 box image with a per-sample value field
    c = Case("33x20", (33, 20), 2, 2, 103)
    c.nu = c.rng.uniform(0.5, 1.5, (1, *c.shp)); c.f = 10 * c.rng.standard_normal((1, *c.shp))
    c.cond = [(box_image(c.shp)[None], c.rng.standard_normal((2, *c.shp)), "f32")]
    cases[c.name] = c
    # D: 65^2 B = 2 -- nu absent, per-sample f, a bit-packed box mask, constant 0
    c = Case("65x65", (65, 65), 2, 2, 104)
    c.f = 10 * c.rng.standard_normal((2, *c.shp))
    c.cond = [(box_image(c.shp)[None], 0.0, "packed")]
    cases[c.name] = c
    # E: 9^3 B = 2 -- per-sample nu and f, a shared uint8 box image with constant 0 and a per-sample fp32 blob with constant 1
    c = Case("9x9x9", (9, 9, 9), 2, 2, 105)
    c.nu = c.rng.uniform(0.5, 1.5, (2, *c.shp)); c.f = 10 * c.rng.standard_normal((2, *c.shp))
    blob = np.zeros((2, *c.shp), bool); blob[0, 4, 3:6, 4] = True; blob[1, 2:4, 5, 5] = True
    c.cond = [(box_image(c.shp)[None], 0.0, "u8"), (blob, 1.0, "f32")]
    cases[c.name] = c
    # F: 17 x 9 x 12 B = 1 -- random nu, forcing at the Gauss points, box faces, random u0
    c = Case("17x9x12", (17, 9, 12), 1, 2, 106)
    c.nu = c.rng.uniform(0.5, 1.5, (1, *c.shp)); c.u0 = c.rng.standard_normal((1, *c.shp))
    c.f_gp = 10 * c.rng.standard_normal((1, c.geom.ngp_total, *c.geom.elem_shape))
    c.cond = [(box_image(c.shp)[None], 0.25, "box")]
    cases[c.name] = c
    return cases


CASES = make_cases()
NAMES = list(CASES)


def solve_case(c, samples=None, **options):
    from diffnet_amd import solve
    kw = c.torch_inputs(samples)
    kw.update(options)
    return solve.poisson_solve(c.geom, **kw)


def fixed_t(c, kw):
    """bool (B,1,*N) tensor of the Dirichlet nodes of the torch conditions"""
    from diffnet_amd import ops
    like = torch.zeros((kw["batch"], 1, *c.shp), device=dev())
    fx = torch.zeros_like(like, dtype=torch.bool)
    for d in kw["dirichlet"]:
        fx = fx | ops._dirichlet_cond(ops._mask_image(d.mask, like))
    return fx


# ---------------------------------------------------------------------------------------------
# 1. the diagonal
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_diagonal_against_float64_and_colour_probing(name):
    from diffnet_amd import ops
    c = CASES[name]
    kw = c.torch_inputs()
    dinv = ops.poisson_diag(c.geom, c.B, kw["nu"], kw["dirichlet"], wscale=c.jac)
    got = dinv.double().cpu().numpy().reshape(c.B, -1)
    worst = 0.0
    for b in range(c.B):
        K, _ = c.system(b)
        fx = sr.fixed_nodes(K.shape[0], c.conditions(b))
        ref = sr.dense_dinv(K, fx)
        assert np.all(got[b][ref == 0] == 0), "dinv must be exactly 0 on Dirichlet nodes and where the diagonal vanishes"
        live = ref != 0
        rel = np.abs(got[b][live] - ref[live]) / ref[live]
        worst = max(worst, rel.max() / U)
        assert rel.max() <= DIAG_ROUNDINGS * U
    print(f"diag {name}: worst error {worst:.1f} x 2^-24 (bound {DIAG_ROUNDINGS})")
    if name == "17x17":
        patch = dinv[2, 0, 6:10, 7:11]
        assert torch.all(patch == 0) and torch.all(dinv[0, 0, 6:10, 7:11] > 0)
    # unit: 1 on exactly the nodes where the Jacobi form is non-zero
    unit = ops.poisson_diag(c.geom, c.B, kw["nu"], kw["dirichlet"], wscale=c.jac, unit=True)
    assert torch.equal(unit, (dinv != 0).float())
    # colour probing: K without conditions applied to the parity indicator fields; the Q1 stencil never joins two nodes of one class
    nsd = c.geom.nsd
    grids = np.indices(c.shp)
    diag = torch.zeros((c.B, 1, *c.shp), device=dev())
    for par in itertools.product((0, 1), repeat=nsd):
        e = np.all([grids[d] % 2 == par[d] for d in range(nsd)], 0).astype(np.float32)
        et = cu(np.broadcast_to(e, (c.B, 1, *c.shp)))
        out, _ = ops.poisson_apply(c.geom, et, kw["nu"], None, None, (), alpha=1.0, beta=0.0, c=0.0, wscale=c.jac, want_out=True, want_sums=False)
        diag += out * et
    livet = dinv != 0
    rel = ((1.0 / dinv[livet]).double() - diag[livet].double()).abs() / diag[livet].double()
    print(f"diag {name}: colour probing, worst {float(rel.max()) / U:.1f} x 2^-24 (bound {PROBE_ROUNDINGS + DIAG_ROUNDINGS})")
    assert float(rel.max()) <= (PROBE_ROUNDINGS + DIAG_ROUNDINGS) * U
    # bitwise the same alone and in a batch
    if c.B > 1:
        for b in range(c.B):
            k1 = c.torch_inputs([b])
            solo = ops.poisson_diag(c.geom, 1, k1["nu"], k1["dirichlet"], wscale=c.jac)
            assert torch.equal(solo[0], dinv[b]), (name, b)


# ---------------------------------------------------------------------------------------------
# 2. the phases one by one
# ---------------------------------------------------------------------------------------------
STATE_FIELDS = ("rz", "rr", "rr0", "pq", "alpha", "beta", "active", "iterations", "flags")


def run_phases(n, B, arrays, tol, atol):
    """INIT, DOT, UPDATE, DIRECTION on copies of the given (B, n) float32 arrays; returns the arrays and the state after every phase."""
    from diffnet_amd import ops
    x, out, q, dinv = (cu(arrays[k]) for k in ("x", "out", "q", "dinv"))
    r, p = torch.full_like(x, 7.0), torch.full_like(x, -3.0)
    state = ops.poisson_cg_state(B, dev())
    ws = ops.poisson_cg_workspace(n, B, dev())
    snap = {}

    def keep(tag):
        snap[tag] = dict(x=x.clone(), r=r.clone(), p=p.clone(), st=ops.poisson_cg_read_state(state).copy())

    ops.poisson_cg_phase("init", x, r, p, out, dinv, state, ws, tol, atol)
    keep("init")
    if "poison" in arrays:                                   # NaN into p and q of the samples that INIT left inactive
        for b in arrays["poison"]:
            p[b] = float("nan"); q[b] = float("nan")
        keep("init")
    ops.poisson_cg_phase("dot", x, r, p, q, dinv, state, ws, tol, atol)
    keep("dot")
    ops.poisson_cg_phase("update", x, r, p, q, dinv, state, ws, tol, atol)
    keep("update")
    ops.poisson_cg_phase("direction", x, r, p, q, dinv, state, ws, tol, atol)
    keep("direction")
    assert not torch.any(ws.view(torch.int32)[: 16 * 65 * B] != 0), "the arrival counters reset themselves"
    return snap


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n", [81, 289, 4225, 70001])
def test_phases_against_float64(n):
    B, tol, atol = 3, 0.5, 0.0
    rng = np.random.default_rng(n)
    A = {k: rng.standard_normal((B, n)).astype(np.float32) for k in ("x", "out", "q")}
    A["dinv"] = np.where(rng.random((B, n)) < 0.1, 0.0, rng.uniform(0.5, 2.0, (B, n))).astype(np.float32)
    A["out"][1] = 0.0                                        # sample 1: rr0 = 0, inactive from INIT on
    A["poison"] = [1]
    # sample 0: q = a positive diagonal times what p will be, plus a little noise: pq > 0.  sample 2: q = -p: pq < 0, breakdown
    p0 = A["dinv"] * -A["out"]
    A["q"][0] = (rng.uniform(0.5, 1.5, n) * p0[0] + 0.01 * rng.standard_normal(n)).astype(np.float32)
    A["q"][2] = -p0[2]
    s = run_phases(n, B, A, tol, atol)
    f64 = lambda t: t.double().cpu().numpy()

    # INIT: r = -out and p = dinv r exactly (one float32 product), the sums to float64 accuracy
    i = s["init"]
    assert np.array_equal(i["r"].cpu().numpy(), -A["out"]) and np.array_equal(np.nan_to_num(i["p"].cpu().numpy(), nan=-1.0)[[0, 2]], p0[[0, 2]])
    r64, p64 = -A["out"].astype(np.float64), p0.astype(np.float64)
    st = i["st"]
    np.testing.assert_allclose(st["rz"], np.sum(r64 * p64, 1), rtol=1e-12)
    np.testing.assert_allclose(st["rr"], np.sum(r64 * r64, 1), rtol=1e-12)
    assert np.array_equal(st["rr0"], st["rr"]) and list(st["active"]) == [1, 0, 1] and not st["iterations"].any() and not st["flags"].any()

    # DOT
    d = s["dot"]["st"]
    pq = np.sum(p64 * A["q"].astype(np.float64), 1)
    np.testing.assert_allclose(d["pq"][[0, 2]], pq[[0, 2]], rtol=1e-12)
    assert pq[0] > 0 > pq[2]
    assert abs(d["alpha"][0] - st["rz"][0] / pq[0]) <= 2 * U * abs(st["rz"][0] / pq[0])
    assert d["alpha"][1] == 0 and d["alpha"][2] == 0
    assert list(d["active"]) == [1, 0, 0] and list(d["flags"]) == [0, 0, 1]
    for k in ("x", "r", "p"):
        assert torch.equal(bits(s["dot"][k]), bits(s["init"][k])), "DOT writes no array"

    # UPDATE (sample 0 alone moves)
    u = s["update"]
    al = float(d["alpha"][0])
    x0, p0_, r0, q0 = A["x"][0].astype(np.float64), p64[0], r64[0], A["q"][0].astype(np.float64)
    assert np.all(np.abs(f64(u["x"][0]) - (x0 + al * p0_)) <= 2 * U * (np.abs(x0) + np.abs(al * p0_)))
    assert np.all(np.abs(f64(u["r"][0]) - (r0 - al * q0)) <= 2 * U * (np.abs(r0) + np.abs(al * q0)))
    rn = f64(u["r"][0])
    zn = (A["dinv"][0] * u["r"][0].cpu().numpy()).astype(np.float64)
    us = u["st"]
    np.testing.assert_allclose(us["rz"][0], np.sum(rn * zn), rtol=1e-12)
    np.testing.assert_allclose(us["rr"][0], np.sum(rn * rn), rtol=1e-12)
    beta = us["rz"][0] / st["rz"][0]
    assert abs(us["beta"][0] - beta) <= 2 * U * abs(beta)
    assert list(us["iterations"]) == [1, 0, 0]
    assert us["active"][0] == int(us["rr"][0] > max(np.float64(np.float32(tol)) ** 2 * us["rr0"][0], atol ** 2))
    assert torch.equal(bits(u["p"]), bits(s["dot"]["p"]))

    # DIRECTION
    g = s["direction"]
    if us["active"][0]:
        want = zn + float(us["beta"][0]) * p0_
        assert np.all(np.abs(f64(g["p"][0]) - want) <= 3 * U * (np.abs(zn) + np.abs(us["beta"][0] * p0_)))
    else:
        assert torch.equal(bits(g["p"][0]), bits(u["p"][0]))
    # the inactive sample (NaN in p and q) and the broken-down one: x, r, p bitwise as they were, no NaN in the scalars
    for b in (1, 2):
        for k in ("x", "r", "p"):
            assert torch.equal(bits(g[k][b]), bits(s["init"][k][b])), (b, k)
        for k in STATE_FIELDS:
            assert np.isfinite(g["st"][k][b]), (b, k)
    assert g["st"]["iterations"][1] == 0 and g["st"]["pq"][1] == 0 and g["st"]["active"][1] == 0

    # run to run, and each sample alone: bitwise the same arrays and scalars
    s2 = run_phases(n, B, A, tol, atol)
    for tag in ("init", "dot", "update", "direction"):
        assert s[tag]["st"].tobytes() == s2[tag]["st"].tobytes()
        for k in ("x", "r", "p"):
            assert torch.equal(bits(s[tag][k]), bits(s2[tag][k]))
    for b in range(B):
        Ab = {k: v[b:b + 1] for k, v in A.items() if k != "poison"}
        if b in A["poison"]:
            Ab["poison"] = [0]
        sb = run_phases(n, 1, Ab, tol, atol)
        for tag in ("init", "dot", "update", "direction"):
            assert sb[tag]["st"][0].tobytes() == s[tag]["st"][b].tobytes(), (b, tag)
            for k in ("x", "r", "p"):
                assert torch.equal(bits(sb[tag][k][0]), bits(s[tag][k][b])), (b, tag, k)


# ---------------------------------------------------------------------------------------------
# 3. + 4. the whole solve against the dense float64 solution; the true residual
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_solve_against_the_dense_solution(name):
    from diffnet_amd import ops, solve
    c = CASES[name]
    kw = c.torch_inputs()
    s = solve.PoissonSolver(c.geom, tol=1e-6, **kw)
    info = s.solve()
    u = s.solution
    assert info.converged.all() and not info.breakdown.any(), (info.iterations, info.rel_residual)
    assert u.shape == (c.B, 1, *c.shp) and torch.isfinite(u).all()
    got = u.double().cpu().numpy().reshape(c.B, -1)
    assert torch.equal(ops._apply_dirichlet(u, kw["dirichlet"]), u), "Dirichlet nodes hold their values exactly"
    # the true residual, recomputed by the existing operator, against the recurrence's: as a vector (|R + r|, which bounds the gap of the
    # two norms | |R| - sqrt(rr) | and, unlike it, cannot vanish by cancellation) relative to |r0|
    R = ops.residual(c.geom, u, kw["nu"], kw["f"], kw.get("f_gp"), kw["dirichlet"], c.jac).double()
    rr_true = (R * R).flatten(1).sum(1).cpu().numpy()
    gaps = (R + s.r.double()).flatten(1).norm(dim=1).cpu().numpy() / np.sqrt(info.rr0)
    worst = worst_gap = 0.0
    for b in range(c.B):
        u64, x32, i32, err32 = c.reference(b)
        assert i32["converged"], "the float32 reference run must reach the tolerance itself"
        err = np.max(np.abs(got[b] - u64)) / np.max(np.abs(u64))
        ratio = err / err32
        worst = max(worst, ratio)
        print(f"solve {name}[{b}]: {info.iterations[b]} iterations (reference {i32['iterations']}), error {err:.3e}, float32 reference {err32:.3e}, ratio {ratio:.2f}")
        assert err <= MARGIN * err32
        # the same gap of the float32 reference run, its true residual evaluated in float32 as the operator evaluates it
        K, rhs = c.system(b)
        fxn = sr.fixed_nodes(len(rhs), c.conditions(b))
        Rref = np.where(fxn, 0, K.astype(np.float32) @ x32.astype(np.float32) - rhs.astype(np.float32)).astype(np.float64)
        gap_ref = np.linalg.norm(Rref + i32["r"]) / np.sqrt(i32["rr0"])
        scalar_gap = abs(np.sqrt(rr_true[b]) - np.sqrt(info.rr[b])) / np.sqrt(info.rr0[b])
        worst_gap = max(worst_gap, gaps[b] / gap_ref)
        print(f"solve {name}[{b}]: true residual against the recurrence: |R + r| = {gaps[b]:.3e} |r0| (norms differ by {scalar_gap:.3e} |r0|), "
              f"float32 reference {gap_ref:.3e}, ratio {gaps[b] / gap_ref:.2f}")
        assert scalar_gap <= gaps[b] * (1 + 1e-6) + 1e-30 and gaps[b] <= MARGIN * gap_ref
        np.testing.assert_allclose(info.rr0[b], i32["rr0"], rtol=1e-4)
    print(f"solve {name}: largest error ratio {worst:.2f}, largest residual-gap ratio {worst_gap:.2f} (margin {MARGIN})")
    # the energy gradient at u* is the residual again, scaled: correspondingly small
    m_scale = c.B * c.geom.nelem_total
    loss, grad = ops.energy_loss_and_grad(c.geom, u, kw["nu"], kw["f"], kw.get("f_gp"), kw["dirichlet"], c=0.5, jac=c.jac)
    gn = (grad.double() * m_scale).flatten(1).norm(dim=1).cpu().numpy()
    assert np.all(gn <= 1.001 * np.sqrt(rr_true) + 1e-30)
    # the energy rises under a random perturbation of the free nodes that carry an equation
    dinv = ops.poisson_diag(c.geom, c.B, kw["nu"], kw["dirichlet"], wscale=c.jac)
    g = torch.Generator(device="cpu").manual_seed(5)
    delta = torch.randn(u.shape, generator=g).to(dev()) * 0.05 * float(u.abs().max())
    delta = torch.where(dinv != 0, delta, torch.zeros_like(delta))
    loss2, _ = ops.energy_loss_and_grad(c.geom, u + delta, kw["nu"], kw["f"], kw.get("f_gp"), kw["dirichlet"], c=0.5, jac=c.jac)
    assert float(loss2) > float(loss)


# ---------------------------------------------------------------------------------------------
# 5. determinism and batch independence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["17x17", "9x9x9", "65x65"])
def test_solve_is_bitwise_reproducible_and_batch_independent(name):
    c = CASES[name]
    u1, i1 = solve_case(c, tol=1e-6)
    u2, i2 = solve_case(c, tol=1e-6)
    assert torch.equal(bits(u1), bits(u2)) and np.array_equal(i1.iterations, i2.iterations) and i1.rr.tobytes() == i2.rr.tobytes()
    if name == "65x65":
        return
    for b in range(c.B):
        us, is_ = solve_case(c, [b], tol=1e-6)
        assert is_.iterations[0] == i1.iterations[b] and is_.rr[0:1].tobytes() == i1.rr[b:b + 1].tobytes(), (name, b)
        assert torch.equal(bits(us[0]), bits(u1[b])), (name, b)


# ---------------------------------------------------------------------------------------------
# 6. control flow
# ---------------------------------------------------------------------------------------------
def test_zero_residual_sample_stands_still_while_its_batch_mates_converge():
    c = CASES["17x17"]
    kw = c.torch_inputs()
    kw["f"] = kw["f"].clone(); kw["f"][0] = 0.0
    kw["dirichlet"][0].value = 0.0
    from diffnet_amd import solve
    u, info = solve.poisson_solve(c.geom, tol=1e-6, **kw)
    assert info.iterations[0] == 0 and info.rr0[0] == 0 and info.converged.all() and info.iterations[1] > 0 and info.iterations[2] > 0
    assert torch.isfinite(u).all() and not u[0].any() and info.rel_residual[0] == 0


def test_maxiter_and_breakdown_end_the_loop():
    c = CASES["33x20"]
    u, info = solve_case(c, tol=1e-6, maxiter=3)
    assert not info.converged.any() and list(info.iterations) == [3, 3] and torch.isfinite(u).all() and info.active.all()
    from diffnet_amd import solve
    kw = c.torch_inputs()
    kw["nu"] = -kw["nu"]
    u, info = solve.poisson_solve(c.geom, tol=1e-6, **kw)
    assert info.breakdown.all() and not info.converged.any() and not info.active.any() and list(info.iterations) == [0, 0]
    assert torch.isfinite(u).all()


def test_jacobi_and_no_preconditioner_reach_the_same_solution():
    c = CASES["17x17"]
    uj, ij = solve_case(c, tol=1e-6)
    un, inn = solve_case(c, tol=1e-6, precondition=None, maxiter=4000)
    assert ij.converged.all() and inn.converged.all()
    for b in range(c.B):
        u64, _, _, err32 = c.reference(b)
        _, _, i32n, err32n = c.reference(b, unit=True) if inn.converged[b] else (None, None, None, err32)
        for tag, u, ref in (("jacobi", uj, err32), ("none", un, err32n)):
            err = np.max(np.abs(u[b].double().cpu().numpy().ravel() - u64)) / np.max(np.abs(u64))
            print(f"precondition {tag} [{b}]: error {err:.3e}, float32 reference {ref:.3e}")
            assert err <= MARGIN * ref
    print("iterations jacobi", ij.iterations, "none", inn.iterations)
    assert ij.iterations[1] <= inn.iterations[1], "Jacobi needs no more iterations on the contrast-100 sample"


# ---------------------------------------------------------------------------------------------
# 7. graph capture, setup() again
# ---------------------------------------------------------------------------------------------
def test_captured_iterations_replay_bitwise_and_setup_picks_up_changes():
    from diffnet_amd import solve
    c = CASES["33x20"]
    kw = c.torch_inputs()
    kw.pop("batch")
    s = solve.PoissonSolver(c.geom, c.B, tol=1e-6, **kw)
    s.setup().iterate(8)
    eager, st_e = s.solution.clone(), s.status()
    assert list(st_e.iterations) == [8, 8]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        s.setup()
        with torch.cuda.graph(graph, stream=side):
            s.iterate(8)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    st_g = s.status()
    assert torch.equal(bits(s.solution), bits(eager)) and st_g.rr.tobytes() == st_e.rr.tobytes() and list(st_g.iterations) == [8, 8]
    # an in-place change of f is picked up by setup()
    kw["f"].mul_(2.0)
    st = s.solve()
    fresh = solve.PoissonSolver(c.geom, c.B, tol=1e-6, **{**kw, "f": kw["f"].clone()})
    st2 = fresh.solve()
    assert st.converged.all() and torch.equal(bits(s.solution), bits(fresh.solution)) and np.array_equal(st.iterations, st2.iterations)
    assert not torch.equal(s.solution, eager)


# ---------------------------------------------------------------------------------------------
# 8. gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes, shared_nu", [((9, 9), False), ((9, 9), True), ((5, 5, 5), False), ((5, 5, 5), True)])
def test_implicit_gradients_against_the_dense_derivative(sizes, shared_nu):
    from diffnet_amd import ops, solve
    B, tol = 2, 1e-7
    geom = geometry(sizes, ngp=2)
    shp = tuple(geom.node_shape)
    rng = np.random.default_rng(sum(sizes) + int(shared_nu))
    jac = float(np.prod([0.5 * h for h in geom.hs]))
    nu = rng.uniform(0.5, 1.5, (1 if shared_nu else B, *shp))
    f = 10 * rng.standard_normal((B, *shp))
    w = rng.standard_normal((B, *shp))
    val = rng.standard_normal((1, *shp))
    box = box_image(shp)
    nu_t, f_t = cu(nu)[:, None].requires_grad_(True), cu(f)[:, None].requires_grad_(True)
    dl = [ops.Dirichlet(cu(box[None, None], torch.uint8), cu(val)[:, None])]
    u, info = solve.poisson_solve(geom, nu_t, f_t, dirichlet=dl, jac=jac, tol=tol)
    assert info.converged.all() and u.requires_grad
    (u * cu(w)[:, None]).sum().backward()
    assert info.adjoint is not None and info.adjoint.converged.all()
    assert nu_t.grad.shape == nu_t.shape and f_t.grad.shape == f_t.shape
    g64 = [np.zeros_like(nu), np.zeros_like(f)]
    g32 = [np.zeros_like(nu), np.zeros_like(f)]
    cond, hom = [(box, val[0])], [(box, 0.0)]
    for b in range(B):
        K, rhs = sr.dense_system(geom, nu[0 if shared_nu else b], f[b], None, jac)
        u64 = sr.dense_solve(K, rhs, cond)
        lam64 = sr.dense_adjoint(K, w[b], cond)
        x32, i32 = sr.cg_restated(K, rhs, cond, tol=tol, dtype=np.float32)
        l32, j32 = sr.cg_restated(K, np.zeros_like(rhs), hom, tol=tol, dtype=np.float32, extra_load=w[b].ravel())
        assert i32["converged"] and j32["converged"]
        for dst, (uu, ll) in ((g64, (u64, lam64)), (g32, (x32, l32))):
            gn, gf = sr.implicit_grads(geom, uu, ll, jac)
            dst[0][0 if shared_nu else b] += gn
            dst[1][b] += gf
    for k, (tag, got) in enumerate((("nu", nu_t.grad), ("f", f_t.grad))):
        got = got[:, 0].double().cpu().numpy()
        scale = np.max(np.abs(g64[k]))
        err, ref = np.max(np.abs(got - g64[k])) / scale, np.max(np.abs(g32[k] - g64[k])) / scale
        print(f"gradient d/d{tag} {sizes} shared_nu={shared_nu}: error {err:.3e}, float32 reference {ref:.3e}, ratio {err / ref:.2f}")
        assert err <= MARGIN * ref
    # signs: a larger coefficient stiffens, d sum(u)/dnu is not all of one sign in general, but d/df of sum(w u) along w K^-1-wise is positive
    lam_dir = f_t.grad.double()
    assert float((lam_dir * (cu(w)[:, None].double())).sum()) > 0


def test_no_gradient_for_value_fields():
    from diffnet_amd import ops, solve
    from diffnet_amd._lib import DiffNetHipError
    geom = geometry((9, 9))
    v = torch.zeros((1, 1, 9, 9), device=dev(), requires_grad=True)
    m = cu(box_image((9, 9))[None, None], torch.uint8)
    with pytest.raises(DiffNetHipError, match="no gradient"):
        solve.poisson_solve(geom, dirichlet=[ops.Dirichlet(m, v)])
    u0 = torch.zeros((1, 1, 9, 9), device=dev(), requires_grad=True)
    with pytest.raises(DiffNetHipError, match="no gradient"):
        solve.poisson_solve(geom, dirichlet=[ops.Dirichlet(m, 0.0)], u0=u0)


# ---------------------------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------------------------
def test_degree_two_is_refused_by_both_layers():
    import ctypes as C
    from diffnet_amd import DiffNet2DFEM, _lib, solve
    from diffnet_amd._lib import DiffNetHipError
    m2 = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    f = torch.ones((1, 1, 9, 9), device=dev())
    with pytest.raises(DiffNetHipError, match="Q1"):
        m2.solve(f=f, dirichlet=[(cu(box_image((9, 9))[None, None], torch.uint8), 0.0)])
    with pytest.raises(DiffNetHipError, match="Q1"):
        solve.PoissonSolver(m2.geom, 1, f=f)
    out = torch.full((1, 1, 9, 9), 3.0, device=dev())
    a = _lib.DnPoissonDiagArgs()
    a.dinv, a.wscale = out.data_ptr(), 1.0
    assert _lib.lib().dn_poisson_diag(C.byref(m2.geom.mesh_struct(1)), C.byref(a), None) == -2
    torch.cuda.synchronize()
    assert torch.all(out == 3.0), "nothing is launched on a bad argument"
