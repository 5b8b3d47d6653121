"""GPU tests of the multigrid preconditioner of the batched CG solve (dn_poisson_mg: csrc/poisson_mg.hip; dn_poisson_pcg:
csrc/poisson_cg.hip; diffnet_amd/solve.py) against the float64 restatement of tests/mg_ref.py:
  1. the transfers and the smoother update alone against the explicit P; the adjoint identity; Dirichlet nodes; batch independence;
  2. the four dn_poisson_pcg phases against float64, with an inactive sample whose arrays hold NaN;
  3. one V-cycle z = M r;
  4. whole solves against the dense solution; Jacobi and multigrid agree; determinism; control flow; graph capture; mask kinds;
     composed against fused;
  5. iteration counts as conditions; 6. implicit gradients; 7. meshes that cannot be coarsened.

Bounds (the convention of tests/test_gpu_solve.py): a float32 result is measured against float64, and its error may be at most MARGIN = 4
times the error of the float32 run of the SAME recurrence in mg_ref / numpy; every test prints the ratio it measured.
Largest observed ratios (MI355X, profiles/poisson_multigrid.txt): transfers 2.08, smoother 1.05, one V-cycle 1.86, solution error 1.08,
residual gap 1.19, gradients 2.30, against the margin of 4; GPU iteration counts equal the float64 restatement's (5, 5, 6)."""
import numpy as np
import pytest
import torch

import mg_ref
import solve_ref as sr
from test_gpu_solve import MARGIN, U, Case, bits, box_image, cu, dev
from test_solve_host import geometry

pytestmark = pytest.mark.gpu


def omega_of(geom):
    from diffnet_amd import solve
    return solve.default_mg_omega(geom)


# ---------------------------------------------------------------------------------------------
# 1. transfers and smoother alone
# ---------------------------------------------------------------------------------------------
# sizes (x, y[, z]) of the fine mesh: 129 x 5 has a coarse row of 65 nodes (it crosses a wave), 131 x 3 one of 66
TRANSFER_SIZES = [(3, 3), (5, 3), (17, 9), (129, 5), (131, 3), (3, 3, 3), (9, 5, 3)]


def run_transfers(shape, B, A, mask_batched):
    """restrict, prolong, smooth0, smooth on copies of the (B, n) arrays of A; masks (1|B, n) bool."""
    from diffnet_amd import ops
    sel = (lambda m: m) if mask_batched else (lambda m: m[:1])
    out = {}
    c = torch.full((B, A["c"].shape[1]), 5.0, device=dev())
    ops.poisson_mg("restrict", shape, B, b=cu(A["b"]), q=cu(A["q"]), c=c, mask=cu(sel(A["cmask"]), torch.uint8))
    out["restrict"] = c
    x = cu(A["x"])
    ops.poisson_mg("prolong", shape, B, x=x, c=cu(A["c"]), mask=cu(sel(A["fmask"]), torch.uint8))
    out["prolong"] = x
    x = torch.full_like(x, 9.0)
    ops.poisson_mg("smooth0", shape, B, x=x, b=cu(A["b"]), dinv=cu(A["dinv"]), omega=0.8)
    out["smooth0"] = x
    x = cu(A["x"])
    ops.poisson_mg("smooth", shape, B, x=x, b=cu(A["b"]), q=cu(A["q"]), dinv=cu(A["dinv"]), omega=0.8)
    out["smooth"] = x
    # without masks, from zero: P e and P^T r themselves
    pe = torch.zeros_like(x)
    ops.poisson_mg("prolong", shape, B, x=pe, c=cu(A["c"]))
    ptr = torch.empty_like(c)
    ops.poisson_mg("restrict", shape, B, b=cu(A["b"]), q=torch.zeros_like(x), c=ptr)
    out["Pe"], out["PTr"] = pe, ptr
    return out


@pytest.mark.parametrize("mask_batched", [False, True])
@pytest.mark.parametrize("sizes", TRANSFER_SIZES)
def test_transfers_and_smoother_against_the_explicit_P(sizes, mask_batched):
    B = 3
    shape = tuple(sizes[::-1])                                # memory order
    cshape = tuple((s - 1) // 2 + 1 for s in shape)
    nf, nc = int(np.prod(shape)), int(np.prod(cshape))
    assert nf % 2 == 1, "odd n: the bases of samples 1 and 2 are only 4-byte aligned"
    rng = np.random.default_rng(nf + int(mask_batched))
    A = {k: rng.standard_normal((B, nf)).astype(np.float32) for k in ("b", "q", "x")}
    A["c"] = rng.standard_normal((B, nc)).astype(np.float32)
    A["dinv"] = np.where(rng.random((B, nf)) < 0.2, 0.0, rng.uniform(0.5, 2.0, (B, nf))).astype(np.float32)
    A["fmask"], A["cmask"] = rng.random((B, nf)) < 0.25, rng.random((B, nc)) < 0.25
    got = run_transfers(shape, B, A, mask_batched)
    P = mg_ref.prolongation(cshape)
    assert P.shape == (nf, nc)
    fm = A["fmask"] if mask_batched else np.repeat(A["fmask"][:1], B, 0)
    cm = A["cmask"] if mask_batched else np.repeat(A["cmask"][:1], B, 0)
    f64 = {k: v.astype(np.float64) for k, v in A.items() if v.dtype == np.float32}
    P32 = P.astype(np.float32)
    om32 = np.float32(0.8)
    om64 = np.float64(om32)
    ref64 = dict(restrict=np.where(cm, 0, (f64["b"] - f64["q"]) @ P), prolong=f64["x"] + np.where(fm, 0, f64["c"] @ P.T),
                 smooth0=om64 * f64["dinv"] * f64["b"], smooth=f64["x"] + om64 * f64["dinv"] * (f64["b"] - f64["q"]),
                 Pe=f64["c"] @ P.T, PTr=f64["b"] @ P)
    ref32 = dict(restrict=np.where(cm, 0, (A["b"] - A["q"]) @ P32), prolong=A["x"] + np.where(fm, 0, A["c"] @ P32.T).astype(np.float32),
                 smooth0=om32 * A["dinv"] * A["b"], smooth=A["x"] + om32 * A["dinv"] * (A["b"] - A["q"]),
                 Pe=A["c"] @ P32.T, PTr=A["b"] @ P32)
    err = {}
    for k, r64 in ref64.items():
        assert ref32[k].dtype == np.float32
        g = got[k].double().cpu().numpy()
        scale = np.max(np.abs(r64))
        e, e32 = np.max(np.abs(g - r64)) / scale, np.max(np.abs(ref32[k].astype(np.float64) - r64)) / scale
        err[k] = (e, e32, scale)
        print(f"{k} {sizes} masks {'per sample' if mask_batched else 'shared'}: error {e:.3e}, float32 reference {e32:.3e}, ratio {e / e32 if e32 else float('inf') if e else 0:.2f}")
        assert e <= MARGIN * e32, k
    # <P e, r> = <e, P^T r> with r = b, in float64 from the float32 results: each side within its own error
    lhs = np.sum(got["Pe"].double().cpu().numpy() * f64["b"], 1)
    rhs = np.sum(f64["c"] * got["PTr"].double().cpu().numpy(), 1)
    slack = MARGIN * (err["Pe"][1] * err["Pe"][2] * np.sum(np.abs(f64["b"]), 1) + err["PTr"][1] * err["PTr"][2] * np.sum(np.abs(f64["c"]), 1))
    print(f"adjoint identity {sizes}: |<Pe,r> - <e,PTr>| = {np.max(np.abs(lhs - rhs)):.3e}, allowed {np.min(slack):.3e}")
    assert np.all(np.abs(lhs - rhs) <= slack)
    # Dirichlet nodes: exactly zero (restrict), bitwise untouched (prolong); dinv == 0 nodes of the smoother likewise
    assert not got["restrict"].cpu().numpy()[cm].any()
    assert np.array_equal(got["prolong"].cpu().numpy()[fm].view(np.int32), A["x"][fm].view(np.int32))
    dead = A["dinv"] == 0
    assert not got["smooth0"].cpu().numpy()[dead].any() and np.array_equal(got["smooth"].cpu().numpy()[dead], A["x"][dead])
    # sample 2 alone: bitwise what it is in the batch
    A1 = {k: v[2:3] for k, v in A.items()}
    if not mask_batched:
        A1["fmask"], A1["cmask"] = A["fmask"][:1], A["cmask"][:1]
    solo = run_transfers(shape, 1, A1, mask_batched)
    for k in got:
        assert torch.equal(bits(solo[k][0]), bits(got[k][2])), k


# ---------------------------------------------------------------------------------------------
# 2. the dn_poisson_pcg phases one by one
# ---------------------------------------------------------------------------------------------
PCG_TAGS = ("resid0", "rz", "direction", "dot", "update", "rz2", "direction2")


def run_pcg_phases(n, B, A, tol, atol):
    """RESID0, RZ, DIRECTION, DOT (dn_poisson_cg's), UPDATE, RZ, DIRECTION on copies of the (B, n) arrays."""
    from diffnet_amd import ops
    x, out, q, z, z2 = (cu(A[k]) for k in ("x", "out", "q", "z", "z2"))
    r, p = torch.full_like(x, 7.0), torch.full_like(x, -3.0)
    state = ops.poisson_cg_state(B, dev())
    ws = ops.poisson_cg_workspace(n, B, dev())
    snap = {}

    def keep(tag):
        snap[tag] = dict(x=x.clone(), r=r.clone(), p=p.clone(), st=ops.poisson_cg_read_state(state).copy())

    ops.poisson_pcg_phase("resid0", x, r, p, out, None, state, ws, tol, atol)
    for b in A.get("poison", ()):                            # NaN into everything a later phase could read of the inactive samples
        p[b] = float("nan"); q[b] = float("nan"); z[b] = float("nan"); z2[b] = float("nan")
    keep("resid0")
    ops.poisson_pcg_phase("rz", None, r, None, None, z, state, ws, tol, atol)
    keep("rz")
    ops.poisson_pcg_phase("direction", None, None, p, None, z, state, None, tol, atol)
    keep("direction")
    ops.poisson_cg_phase("dot", None, None, p, q, None, state, ws, tol, atol)
    keep("dot")
    ops.poisson_pcg_phase("update", x, r, p, q, None, state, ws, tol, atol)
    keep("update")
    ops.poisson_pcg_phase("rz", None, r, None, None, z2, state, ws, tol, atol)
    keep("rz2")
    ops.poisson_pcg_phase("direction", None, None, p, None, z2, state, None, tol, atol)
    keep("direction2")
    assert not torch.any(ws.view(torch.int32)[: 16 * 65 * B] != 0), "the arrival counters reset themselves"
    return snap


@pytest.mark.parametrize("n", [81, 289, 4225, 70001])
def test_pcg_phases_against_float64(n):
    B, tol, atol = 3, 0.5, 0.0
    rng = np.random.default_rng(n)
    A = {k: rng.standard_normal((B, n)).astype(np.float32) for k in ("x", "out")}
    A["out"][1] = 0.0                                        # sample 1: rr0 = 0, inactive from RESID0 on
    A["poison"] = [1]
    r0 = -A["out"]
    # z = a positive diagonal times r (rz > 0), q = a positive diagonal times what p will be (= z) plus noise: pq > 0; sample 2: q = -p
    A["z"] = (rng.uniform(0.5, 2.0, (B, n)) * r0).astype(np.float32)
    A["z2"] = rng.standard_normal((B, n)).astype(np.float32)
    A["q"] = (rng.uniform(0.5, 1.5, (B, n)) * A["z"] + 0.01 * rng.standard_normal((B, n))).astype(np.float32)
    A["q"][2] = -A["z"][2]
    s = run_pcg_phases(n, B, A, tol, atol)
    f64 = lambda t: t.double().cpu().numpy()
    d64 = {k: v.astype(np.float64) for k, v in A.items() if k != "poison"}

    # RESID0: r = -out exactly; the sums to float64 accuracy; rz = 0
    i = s["resid0"]
    assert np.array_equal(i["r"].cpu().numpy(), r0)
    st = i["st"]
    np.testing.assert_allclose(st["rr"], np.sum(d64["out"] ** 2, 1), rtol=1e-12)
    assert np.array_equal(st["rr0"], st["rr"]) and list(st["active"]) == [1, 0, 1] and not st["iterations"].any() and not st["flags"].any()
    assert not st["rz"].any() and not st["alpha"].any() and not st["beta"].any()
    assert torch.equal(bits(i["x"]), bits(cu(A["x"]))), "RESID0 writes r alone"
    # RZ after RESID0: rz = sum r z, beta = 0
    t = s["rz"]["st"]
    rz0 = np.sum(r0.astype(np.float64) * d64["z"], 1)
    np.testing.assert_allclose(t["rz"][[0, 2]], rz0[[0, 2]], rtol=1e-12)
    assert t["rz"][1] == 0 and not t["beta"].any() and rz0[0] > 0
    # DIRECTION with beta = 0: p = z exactly, whatever p held; the inactive sample's p stays (NaN) as it is
    g = s["direction"]
    assert np.array_equal(g["p"].cpu().numpy()[[0, 2]], A["z"][[0, 2]])
    assert torch.equal(bits(g["p"][1]), bits(s["resid0"]["p"][1]))
    # DOT (unchanged entry): alpha = rz / pq; sample 2 breaks down
    d = s["dot"]["st"]
    pq = np.sum(d64["z"] * d64["q"], 1)
    np.testing.assert_allclose(d["pq"][[0, 2]], pq[[0, 2]], rtol=1e-12)
    assert pq[0] > 0 > pq[2]
    assert abs(d["alpha"][0] - t["rz"][0] / pq[0]) <= 2 * U * abs(t["rz"][0] / pq[0])
    assert list(d["active"]) == [1, 0, 0] and list(d["flags"]) == [0, 0, 1] and d["alpha"][1] == 0 and d["alpha"][2] == 0
    # UPDATE (sample 0 alone moves)
    u = s["update"]
    al = float(d["alpha"][0])
    x0, p0, q0 = d64["x"][0], d64["z"][0], d64["q"][0]
    r00 = r0[0].astype(np.float64)
    assert np.all(np.abs(f64(u["x"][0]) - (x0 + al * p0)) <= 2 * U * (np.abs(x0) + np.abs(al * p0)))
    assert np.all(np.abs(f64(u["r"][0]) - (r00 - al * q0)) <= 2 * U * (np.abs(r00) + np.abs(al * q0)))
    rn = f64(u["r"][0])
    us = u["st"]
    np.testing.assert_allclose(us["rr"][0], np.sum(rn * rn), rtol=1e-12)
    assert list(us["iterations"]) == [1, 0, 0] and us["rz"][0] == t["rz"][0], "UPDATE leaves rz to RZ"
    assert us["active"][0] == int(us["rr"][0] > max(np.float64(np.float32(tol)) ** 2 * us["rr0"][0], atol ** 2))
    assert torch.equal(bits(u["p"]), bits(s["dot"]["p"]))
    # RZ again: beta = rz' / rz; DIRECTION: p = z2 + beta p
    v = s["rz2"]["st"]
    g2 = s["direction2"]
    if us["active"][0]:
        rz1 = np.sum(rn * d64["z2"][0])
        np.testing.assert_allclose(v["rz"][0], rz1, rtol=1e-9, atol=1e-12 * np.sum(np.abs(rn * d64["z2"][0])))
        beta = v["rz"][0] / t["rz"][0]
        assert abs(v["beta"][0] - beta) <= 2 * U * abs(beta)
        want = d64["z2"][0] + float(v["beta"][0]) * p0
        assert np.all(np.abs(f64(g2["p"][0]) - want) <= 3 * U * (np.abs(d64["z2"][0]) + np.abs(v["beta"][0] * p0)))
    else:
        assert v["rz"][0] == us["rz"][0] and torch.equal(bits(g2["p"][0]), bits(u["p"][0]))
    for k in ("x", "r"):
        assert torch.equal(bits(g2[k]), bits(u[k])), "RZ and DIRECTION write p alone"
    # the inactive sample (NaN in p, q, z) and the broken-down one: x, r, p bitwise as they were, no NaN in the scalars
    for b in (1, 2):
        for k in ("x", "r", "p"):
            assert torch.equal(bits(g2[k][b]), bits(s["direction"][k][b])), (b, k)
        for k in ("rz", "rr", "rr0", "pq", "alpha", "beta", "active", "iterations", "flags"):
            assert np.isfinite(g2["st"][k][b]), (b, k)
    assert g2["st"]["iterations"][1] == 0 and g2["st"]["pq"][1] == 0 and g2["st"]["active"][1] == 0 and g2["st"]["rz"][1] == 0
    # run to run, and each sample alone: bitwise the same arrays and scalars
    s2 = run_pcg_phases(n, B, A, tol, atol)
    for tag in PCG_TAGS:
        assert s[tag]["st"].tobytes() == s2[tag]["st"].tobytes()
        for k in ("x", "r", "p"):
            assert torch.equal(bits(s[tag][k]), bits(s2[tag][k]))
    for b in range(B):
        Ab = {k: v[b:b + 1] for k, v in A.items() if k != "poison"}
        if b in A["poison"]:
            Ab["poison"] = [0]
        sb = run_pcg_phases(n, 1, Ab, tol, atol)
        for tag in PCG_TAGS:
            assert sb[tag]["st"][0].tobytes() == s[tag]["st"][b].tobytes(), (b, tag)
            for k in ("x", "r", "p"):
                assert torch.equal(bits(sb[tag][k][0]), bits(s[tag][k][b])), (b, tag, k)


# ---------------------------------------------------------------------------------------------
# cases shared by the V-cycle and solve tests: the references are computed once
# ---------------------------------------------------------------------------------------------
def disk_image(shp, frac=0.22):
    grids = np.indices(shp)
    centre = [(s - 1) * 0.5 + 0.3 for s in shp]
    return sum((grids[d] - centre[d]) ** 2 for d in range(len(shp))) <= (frac * min(shp)) ** 2


class MgCase(Case):
    """A Case of tests/test_gpu_solve.py with the multigrid references of mg_ref beside the Jacobi ones."""

    def levels(self, b):
        key = ("levels", b if ((self.nu is not None and self.nu.shape[0] > 1) or any(m.shape[0] > 1 for m, _, _ in self.cond)) else 0)
        if key not in self._ref:
            fx = sr.fixed_nodes(int(np.prod(self.shp)), self.conditions(b))
            self._ref[key] = mg_ref.hierarchy(self.geom, self.pick(self.nu, b), fx, self.jac)
        return self._ref[key]

    def mg_reference(self, b, tol=1e-6):
        """(u64, x32, info32, err32, info64): the dense solution, mg_ref.pcg's float32 run and its error, the float64 run's info."""
        key = ("mgref", b, tol)
        if key not in self._ref:
            K, rhs = self.system(b)
            cond, x0 = self.conditions(b), self.pick(self.u0, b)
            u64 = sr.dense_solve(K, rhs, cond, x0)
            kw = dict(levels=self.levels(b), tol=tol, omega=omega_of(self.geom), maxiter=200)
            x32, i32 = mg_ref.pcg(K, rhs, cond, x0, dtype=np.float32, **kw)
            _, i64 = mg_ref.pcg(K, rhs, cond, x0, **kw)
            self._ref[key] = (u64, x32, i32, np.max(np.abs(x32 - u64)) / max(np.max(np.abs(u64)), 1e-300), i64)
        return self._ref[key]


def make_cases():
    cases = {}

    def add(name, sizes, B, seed, kind, form="box", ngp=2):
        c = MgCase(name, sizes, B, ngp, seed)
        c.f = 10 * c.rng.standard_normal((B, *c.shp))
        box = box_image(c.shp)[None]
        if kind == "box":                                    # box faces alone, nu absent
            c.cond = [(box, 0.0, form)]
        elif kind == "disk":                                 # box faces plus an immersed disk with a value, shared nu
            c.nu = c.rng.uniform(0.5, 1.5, (1, *c.shp))
            c.cond = [(box, 0.0, form), (disk_image(c.shp)[None], 0.75, "f32")]
        else:                                                # random per-sample nu, a value field on the box, random u0
            c.nu = c.rng.uniform(0.5, 1.5, (B, *c.shp))
            c.u0 = c.rng.standard_normal((1, *c.shp))
            c.cond = [(box, c.rng.standard_normal((1, *c.shp)), form)]
        cases[name] = c

    for sizes in ((9, 9), (17, 9), (13, 9), (9, 9, 9)):
        tag = "x".join(map(str, sizes))
        add(tag + "-box", sizes, 1, 201, "box")
        add(tag + "-disk", sizes, 2, 202, "disk", "u8")
        add(tag + "-nu", sizes, 2, 203, "nu", "f32")
    add("17x17-nu", (17, 17), 2, 204, "nu", "u8", ngp=3)
    add("65x65-box", (65, 65), 1, 205, "box", "packed")
    add("17x17x17-disk", (17, 17, 17), 1, 206, "disk")
    add("33x17-nu", (33, 17), 2, 207, "nu", "f32")
    return cases


CASES = make_cases()
VCYCLE_NAMES = [n for n in CASES if n.split("-")[0] in ("9x9", "17x9", "13x9", "9x9x9")]


# ---------------------------------------------------------------------------------------------
# 3. one V-cycle
# ---------------------------------------------------------------------------------------------
OTHER_CYCLE = dict(mg_sweeps=2, mg_coarse_sweeps=1, mg_max_levels=2)
VCYCLES = [(n, {}) for n in VCYCLE_NAMES] + [(n, OTHER_CYCLE) for n in VCYCLE_NAMES if n.endswith("-nu")]


@pytest.mark.parametrize("name, options", VCYCLES, ids=[n + ("-2sweeps-2levels" if o else "") for n, o in VCYCLES])
def test_one_vcycle_against_the_restatement(name, options):
    from diffnet_amd import solve
    c = CASES[name]
    kw = c.torch_inputs()
    B = kw.pop("batch")
    s = solve.PoissonSolver(c.geom, B, **kw, precondition="multigrid", **options).setup()
    assert len(s.mg.levels) == min(len(mg_ref.level_shapes(c.shp)), options.get("mg_max_levels", 99))
    rng = np.random.default_rng(5)
    r = rng.standard_normal((B, *c.shp))
    for b in range(B):
        r[b][sr.fixed_nodes(r[b].size, c.conditions(b)).reshape(c.shp)] = 0.0       # a CG residual is zero on the Dirichlet nodes
    r = r.astype(np.float32)
    z = s.apply_preconditioner(cu(r)[:, None])
    zc = solve.PoissonSolver(c.geom, B, **kw, precondition="multigrid", phases="composed", **options).setup().apply_preconditioner(cu(r)[:, None])
    mgkw = dict(sweeps=options.get("mg_sweeps", 1), omega=omega_of(c.geom), coarse_sweeps=options.get("mg_coarse_sweeps", 4))
    for b in range(B):
        lv = c.levels(b)[: options.get("mg_max_levels")]
        z64 = mg_ref.vcycle(lv, r[b].ravel(), **mgkw)
        z32 = mg_ref.vcycle(lv, r[b].ravel(), dtype=np.float32, **mgkw)
        assert z32.dtype == np.float32
        scale = np.max(np.abs(z64))
        e32 = np.max(np.abs(z32 - z64)) / scale
        for tag, t in (("fused", z), ("composed", zc)):
            got = t[b].double().cpu().numpy().ravel()
            e = np.max(np.abs(got - z64)) / scale
            print(f"V-cycle {name}[{b}] {tag}: error {e:.3e}, float32 reference {e32:.3e}, ratio {e / e32:.2f}")
            assert e <= MARGIN * e32, (tag, b)
            assert not got[lv[0]["fixed"]].any(), "z is zero on the Dirichlet nodes"


# ---------------------------------------------------------------------------------------------
# 4. whole solves
# ---------------------------------------------------------------------------------------------
def mg_solve(c, samples=None, **options):
    from diffnet_amd import solve
    kw = c.torch_inputs(samples)
    kw.update(options)
    return solve.poisson_solve(c.geom, precondition="multigrid", **kw)


@pytest.mark.parametrize("name", ["17x17-nu", "65x65-box", "9x9x9-nu", "17x17x17-disk"])
def test_multigrid_solve_against_the_dense_solution(name):
    from diffnet_amd import ops, solve
    c = CASES[name]
    kw = c.torch_inputs()
    s = solve.PoissonSolver(c.geom, tol=1e-6, precondition="multigrid", **kw)
    info = s.solve()
    u = s.solution
    assert info.converged.all() and not info.breakdown.any(), (info.iterations, info.rel_residual)
    assert u.shape == (c.B, 1, *c.shp) and torch.isfinite(u).all()
    assert torch.equal(ops._apply_dirichlet(u, kw["dirichlet"]), u), "Dirichlet nodes hold their values exactly"
    got = u.double().cpu().numpy().reshape(c.B, -1)
    R = ops.residual(c.geom, u, kw["nu"], kw["f"], kw.get("f_gp"), kw["dirichlet"], c.jac).double()
    gaps = (R + s.r.double()).flatten(1).norm(dim=1).cpu().numpy() / np.sqrt(info.rr0)
    for b in range(c.B):
        u64, x32, i32, err32, i64 = c.mg_reference(b)
        assert i32["converged"], "the float32 reference run must reach the tolerance itself"
        err = np.max(np.abs(got[b] - u64)) / np.max(np.abs(u64))
        print(f"multigrid solve {name}[{b}]: {info.iterations[b]} iterations (float32 reference {i32['iterations']}, float64 {i64['iterations']}), "
              f"error {err:.3e}, float32 reference {err32:.3e}, ratio {err / err32:.2f}")
        assert err <= MARGIN * err32
        K, rhs = c.system(b)
        fxn = sr.fixed_nodes(len(rhs), c.conditions(b))
        Rref = np.where(fxn, 0, K.astype(np.float32) @ x32.astype(np.float32) - rhs.astype(np.float32)).astype(np.float64)
        gap_ref = np.linalg.norm(Rref + i32["r"]) / np.sqrt(i32["rr0"])
        print(f"multigrid solve {name}[{b}]: true residual against the recurrence |R + r| = {gaps[b]:.3e} |r0|, float32 reference {gap_ref:.3e}, ratio {gaps[b] / gap_ref:.2f}")
        assert gaps[b] <= MARGIN * gap_ref
        np.testing.assert_allclose(info.rr0[b], i32["rr0"], rtol=1e-4)


def test_multigrid_and_jacobi_reach_the_same_solution():
    from diffnet_amd import solve
    c = CASES["17x17-nu"]
    um, im = mg_solve(c, tol=1e-6)
    kw = c.torch_inputs()
    uj, ij = solve.poisson_solve(c.geom, tol=1e-6, precondition="jacobi", **kw)
    assert im.converged.all() and ij.converged.all()
    for b in range(c.B):
        u64, _, _, err32m, _ = c.mg_reference(b)
        _, _, _, err32j = c.reference(b)
        for tag, u, ref in (("multigrid", um, err32m), ("jacobi", uj, err32j)):
            err = np.max(np.abs(u[b].double().cpu().numpy().ravel() - u64)) / np.max(np.abs(u64))
            print(f"precondition {tag} [{b}]: error {err:.3e}, float32 reference {ref:.3e}")
            assert err <= MARGIN * ref
    print("iterations multigrid", im.iterations, "jacobi", ij.iterations)
    assert np.all(im.iterations < ij.iterations)


@pytest.mark.parametrize("name", ["17x17-nu", "9x9x9-disk"])
def test_multigrid_solve_is_bitwise_reproducible_and_batch_independent(name):
    c = CASES[name]
    u1, i1 = mg_solve(c, tol=1e-6)
    u2, i2 = mg_solve(c, tol=1e-6)
    assert i1.converged.all()
    assert torch.equal(bits(u1), bits(u2)) and np.array_equal(i1.iterations, i2.iterations) and i1.rr.tobytes() == i2.rr.tobytes()
    for b in range(c.B):
        us, is_ = mg_solve(c, [b], tol=1e-6)
        assert is_.iterations[0] == i1.iterations[b] and is_.rr[0:1].tobytes() == i1.rr[b:b + 1].tobytes(), (name, b)
        assert torch.equal(bits(us[0]), bits(u1[b])), (name, b)


def test_zero_residual_sample_stands_still_under_multigrid():
    from diffnet_amd import solve
    c = CASES["17x9-disk"]
    kw = c.torch_inputs()
    kw["f"] = kw["f"].clone(); kw["f"][0] = 0.0
    for d in kw["dirichlet"]:
        d.value = 0.0
    u, info = solve.poisson_solve(c.geom, tol=1e-6, precondition="multigrid", **kw)
    assert info.iterations[0] == 0 and info.rr0[0] == 0 and info.converged.all() and info.iterations[1] > 0
    assert torch.isfinite(u).all() and not u[0].any() and info.rel_residual[0] == 0


def test_captured_multigrid_iterations_replay_bitwise_and_setup_picks_up_nu():
    from diffnet_amd import solve
    c = CASES["33x17-nu"]
    kw = c.torch_inputs()
    kw.pop("batch")
    s = solve.PoissonSolver(c.geom, c.B, tol=1e-6, precondition="multigrid", **kw)
    s.setup().iterate(3)
    eager, st_e = s.solution.clone(), s.status()
    assert list(st_e.iterations) == [3, 3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        s.setup()
        with torch.cuda.graph(graph, stream=side):
            s.iterate(3)
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    st_g = s.status()
    assert torch.equal(bits(s.solution), bits(eager)) and st_g.rr.tobytes() == st_e.rr.tobytes() and list(st_g.iterations) == [3, 3]
    # an in-place change of nu reaches every level through setup()
    coarse_before = s.mg.levels[1].dinv.clone()
    kw["nu"].mul_(3.0)
    st = s.solve()
    fresh = solve.PoissonSolver(c.geom, c.B, tol=1e-6, precondition="multigrid", **{**kw, "nu": kw["nu"].clone()})
    st2 = fresh.solve()
    assert st.converged.all() and torch.equal(bits(s.solution), bits(fresh.solution)) and np.array_equal(st.iterations, st2.iterations)
    assert not torch.equal(s.mg.levels[1].dinv, coarse_before) and not torch.equal(s.solution, eager)


def test_all_three_mask_kinds_give_the_same_multigrid_solve():
    from diffnet_amd import ops, solve
    c = CASES["17x9-box"]
    kw = c.torch_inputs()
    img = cu(box_image(c.shp)[None, None], torch.uint8)
    sols = {}
    for kind, mask in (("box", ops.BoxFaces("all")), ("packed", ops.PackedMask.pack(img)), ("u8", img), ("f32", img.float())):
        kw["dirichlet"] = [ops.Dirichlet(mask, 0.0)]
        sols[kind], info = solve.poisson_solve(c.geom, tol=1e-6, precondition="multigrid", **kw)
        assert info.converged.all(), kind
    u64, _, _, err32, _ = c.mg_reference(0)
    for kind, u in sols.items():
        err = np.max(np.abs(u[0].double().cpu().numpy().ravel() - u64)) / np.max(np.abs(u64))
        print(f"mask kind {kind}: error {err:.3e}, float32 reference {err32:.3e}")
        assert err <= MARGIN * err32


@pytest.mark.parametrize("name", ["17x9-disk", "9x9x9-nu"])
def test_composed_multigrid_agrees_with_fused(name):
    c = CASES[name]
    uf, i_f = mg_solve(c, tol=1e-6)
    uc, ic = mg_solve(c, tol=1e-6, phases="composed")
    assert i_f.converged.all() and ic.converged.all()
    print("iterations fused", i_f.iterations, "composed", ic.iterations)
    assert np.all(np.abs(i_f.iterations.astype(int) - ic.iterations.astype(int)) <= 1)
    for b in range(c.B):
        u64, _, _, err32, _ = c.mg_reference(b)
        for tag, u in (("fused", uf), ("composed", uc)):
            err = np.max(np.abs(u[b].double().cpu().numpy().ravel() - u64)) / np.max(np.abs(u64))
            print(f"{name}[{b}] {tag}: error {err:.3e}, float32 reference {err32:.3e}")
            assert err <= MARGIN * err32


# ---------------------------------------------------------------------------------------------
# 5. iteration counts: conditions, not timings
# ---------------------------------------------------------------------------------------------
# mg_ref's float64 counts at tol = 1e-5 for the inputs below are 5, 5 and 6 at 17^2, 33^2 and 65^2 (default cycle: one sweep, omega
# 8/9, four coarse sweeps): the count grows by 1 over a 16-fold growth of the mesh.  The margin allowed for that growth is 2.
GROWTH_MARGIN = 2
COUNTS = {}


def count_case(n):
    if n not in COUNTS:
        g = geometry((n, n))
        rng = np.random.default_rng(n)
        nu, f = rng.uniform(0.5, 1.5, g.node_shape), rng.standard_normal(g.node_shape)
        box = box_image(tuple(g.node_shape))
        K, b = sr.dense_system(g, nu, f)
        _, info = mg_ref.pcg(K, b, [(box, 0.0)], levels=mg_ref.hierarchy(g, nu, box), tol=1e-5, omega=omega_of(g))
        assert info["converged"]
        COUNTS[n] = (g, nu, f, info["iterations"])
    return COUNTS[n]


@pytest.mark.parametrize("n", [17, 33, 65])
def test_iteration_count_against_the_float64_restatement(n):
    from diffnet_amd import ops, solve
    g, nu, f, ref_its = count_case(n)
    u, info = solve.poisson_solve(g, cu(nu)[None, None], cu(f)[None, None], dirichlet=[ops.Dirichlet(ops.BoxFaces("all"), 0.0)], tol=1e-5,
                                  precondition="multigrid", check_every=1)
    print(f"{n}^2: {info.iterations[0]} iterations, float64 restatement {ref_its}")
    assert info.converged.all() and info.iterations[0] <= ref_its + 2      # 2: float32 rounding of alpha and beta


def test_reference_iteration_count_is_mesh_independent():
    its = {n: count_case(n)[3] for n in (17, 65)}
    print("float64 restatement iterations", its)
    assert its[65] <= its[17] + GROWTH_MARGIN


def test_multigrid_needs_fewer_iterations_than_jacobi_on_a_contrast_case():
    from diffnet_amd import ops, solve
    n = 65
    g = geometry((n, n))
    y, x = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    nu = np.exp(np.log(0.2) + (np.log(50.0) - np.log(0.2)) * 0.5 * (1 + np.sin(2 * np.pi * x) * np.cos(3 * np.pi * y)))
    assert 0.19 < nu.min() < 0.3 and 35 < nu.max() < 51
    f = np.random.default_rng(3).standard_normal((n, n))
    its = {}
    for pre in ("multigrid", "jacobi"):
        u, info = solve.poisson_solve(g, cu(nu)[None, None], cu(f)[None, None], dirichlet=[ops.Dirichlet(ops.BoxFaces("all"), 0.0)], tol=1e-5,
                                      precondition=pre, check_every=1)
        assert info.converged.all(), pre
        its[pre] = int(info.iterations[0])
    print("contrast 0.2 .. 50 at 65^2:", its)
    assert its["multigrid"] < its["jacobi"]


# ---------------------------------------------------------------------------------------------
# 6. implicit gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(9, 9), (5, 5, 5)])
def test_implicit_gradients_with_multigrid_against_the_dense_derivative(sizes):
    from diffnet_amd import ops, solve
    B, tol = 2, 1e-7
    geom = geometry(sizes, ngp=2)
    shp = tuple(geom.node_shape)
    rng = np.random.default_rng(sum(sizes))
    jac = float(np.prod([0.5 * h for h in geom.hs]))
    nu, f, w = rng.uniform(0.5, 1.5, (B, *shp)), 10 * rng.standard_normal((B, *shp)), rng.standard_normal((B, *shp))
    val = rng.standard_normal((1, *shp))
    box = box_image(shp)
    nu_t, f_t = cu(nu)[:, None].requires_grad_(True), cu(f)[:, None].requires_grad_(True)
    dl = [ops.Dirichlet(cu(box[None, None], torch.uint8), cu(val)[:, None])]
    u, info = solve.poisson_solve(geom, nu_t, f_t, dirichlet=dl, jac=jac, tol=tol, precondition="multigrid")
    assert info.converged.all() and u.requires_grad
    (u * cu(w)[:, None]).sum().backward()
    assert info.adjoint is not None and info.adjoint.converged.all(), "the adjoint solve goes through the same solver"
    g64, g32 = [np.zeros_like(nu), np.zeros_like(f)], [np.zeros_like(nu), np.zeros_like(f)]
    cond, hom = [(box, val[0])], [(box, 0.0)]
    om = omega_of(geom)
    for b in range(B):
        K, rhs = sr.dense_system(geom, nu[b], f[b], None, jac)
        lv = mg_ref.hierarchy(geom, nu[b], box, jac)
        u64, lam64 = sr.dense_solve(K, rhs, cond), sr.dense_adjoint(K, w[b], cond)
        x32, i32 = mg_ref.pcg(K, rhs, cond, levels=lv, tol=tol, dtype=np.float32, omega=om)
        l32, j32 = mg_ref.pcg(K, np.zeros_like(rhs), hom, levels=lv, tol=tol, dtype=np.float32, extra_load=w[b].ravel(), omega=om)
        assert i32["converged"] and j32["converged"]
        for dst, (uu, ll) in ((g64, (u64, lam64)), (g32, (x32, l32))):
            gn, gf = sr.implicit_grads(geom, uu, ll, jac)
            dst[0][b] += gn
            dst[1][b] += gf
    for k, (tag, got) in enumerate((("nu", nu_t.grad), ("f", f_t.grad))):
        got = got[:, 0].double().cpu().numpy()
        scale = np.max(np.abs(g64[k]))
        err, ref = np.max(np.abs(got - g64[k])) / scale, np.max(np.abs(g32[k] - g64[k])) / scale
        print(f"multigrid gradient d/d{tag} {sizes}: error {err:.3e}, float32 reference {ref:.3e}, ratio {err / ref:.2f}")
        assert err <= MARGIN * ref


# ---------------------------------------------------------------------------------------------
# 7. meshes that cannot be coarsened
# ---------------------------------------------------------------------------------------------
def test_meshes_that_cannot_be_coarsened_raise_from_every_entry():
    from diffnet_amd import DiffNet2DFEM, solve
    from diffnet_amd._lib import DiffNetHipError
    m = DiffNet2DFEM(None, domain_size=8)
    f = torch.ones((1, 1, 8, 8), device=dev())
    dl = [(cu(box_image((8, 8))[None, None], torch.uint8), 0.0)]
    with pytest.raises(DiffNetHipError, match="cannot be coarsened"):
        solve.PoissonSolver(m.geom, 1, f=f, dirichlet=dl, precondition="multigrid")
    with pytest.raises(DiffNetHipError, match="cannot be coarsened"):
        solve.poisson_solve(m.geom, f=f, dirichlet=dl, precondition="multigrid")
    with pytest.raises(DiffNetHipError, match="cannot be coarsened"):
        m.solve(f=f, dirichlet=dl, precondition="multigrid")
    u, info = m.solve(f=f, dirichlet=dl)                     # Jacobi as before
    assert info.converged.all()
    m9 = DiffNet2DFEM(None, domain_size=9)
    f9 = torch.ones((1, 1, 9, 9), device=dev())
    u9, i9 = m9.solve(f=f9, dirichlet=[(cu(box_image((9, 9))[None, None], torch.uint8), 0.0)], precondition="multigrid")
    assert i9.converged.all() and torch.isfinite(u9).all()
