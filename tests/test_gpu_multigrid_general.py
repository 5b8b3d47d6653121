"""GPU tests of multigrid on meshes that need not be nested (mg_coarsening="general": dn_poisson_mg_transfer in
csrc/poisson_mg_general.hip, diffnet_amd/solve.py) against the float64 restatement of tests/mg_general_ref.py:
  a. the two transfers alone against the explicit P; the adjoint identity; Dirichlet nodes; batch independence; bad arguments;
  b. one V-cycle z = M r;
  c. whole solves against the dense solution; Jacobi and multigrid agree; a nested mesh solves bitwise the same under both rules;
     determinism; graph capture; mask kinds; composed against fused; the facade;
  d. iteration counts as conditions; e. implicit gradients.

Bounds (the convention of tests/test_gpu_solve.py): a float32 result is measured against float64, and its error may be at most MARGIN = 4
times the error of the float32 run of the SAME statement in the reference; every test prints the ratio it measured.  The float64 side
uses the exact weights of the integer rule, the float32 side the float32-rounded weights the kernels read.  The float32 run of a
transfer applies the per-axis float32 matrices one axis after the other, x first, term by term in index order, as the kernels do.
Largest observed ratios (MI355X, profiles/poisson_multigrid_general.txt): transfers 1.68 (P^T r at 8 x 8; restrict 1.51 at 9 x 8 x 5, prolong
and P e at most 1.15), one V-cycle 2.61 (6 x 7 x 10, two levels; fused and composed alike), solution error 1.09, residual gap 1.29, gradients
1.40, against the margin of 4; GPU iteration counts equal the float64 restatement's (5, 5, 5 at 16^2, 32^2, 64^2; Jacobi 115 at 64^2)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mg_general_ref as gr
import mg_ref
import solve_ref as sr
from test_gpu_multigrid import MgCase, disk_image, omega_of
from test_gpu_solve import MARGIN, bits, box_image, cu, dev
from test_mg_general_host import GROWTH_MARGIN, reference_count
from test_solve_host import geometry

pytestmark = pytest.mark.gpu

GENERAL = dict(precondition="multigrid", mg_coarsening="general")


# ---------------------------------------------------------------------------------------------
# a. the transfers alone
# ---------------------------------------------------------------------------------------------
# sizes (x, y[, z]) of the fine mesh: 9 x 8 has one nested and one general axis, 130 x 4 a coarse row of 66 nodes (it crosses a wave),
# 128 x 6 a fine row of two waves exactly, 259 x 4 a fine row that crosses a workgroup
TRANSFER_SIZES = [(4, 4), (6, 4), (8, 8), (9, 8), (16, 7), (130, 4), (128, 6), (259, 4), (4, 4, 4), (6, 7, 10), (9, 8, 5)]


def run_transfers(shape, B, A, mask_batched, tables=None):
    """restrict and prolong on copies of the (B, n) arrays of A; masks (1|B, n) bool."""
    from diffnet_amd import ops
    tables = tables or ops.MgTransferTables(shape, dev())
    sel = (lambda m: m) if mask_batched else (lambda m: m[:1])
    out = {}
    c = torch.full((B, A["c"].shape[1]), 5.0, device=dev())
    ops.poisson_mg_transfer("restrict", shape, B, tables, b=cu(A["b"]), q=cu(A["q"]), c=c, mask=cu(sel(A["cmask"]), torch.uint8))
    out["restrict"] = c
    x = cu(A["x"])
    ops.poisson_mg_transfer("prolong", shape, B, tables, x=x, c=cu(A["c"]), mask=cu(sel(A["fmask"]), torch.uint8))
    out["prolong"] = x
    # without masks: c and x themselves, then from zero P e and P^T r
    c2 = torch.full_like(c, 5.0)
    ops.poisson_mg_transfer("restrict", shape, B, tables, b=cu(A["b"]), q=cu(A["q"]), c=c2)
    x2 = cu(A["x"])
    ops.poisson_mg_transfer("prolong", shape, B, tables, x=x2, c=cu(A["c"]))
    out["restrict_nomask"], out["prolong_nomask"] = c2, x2
    pe = torch.zeros_like(x)
    ops.poisson_mg_transfer("prolong", shape, B, tables, x=pe, c=cu(A["c"]))
    ptr = torch.empty_like(c)
    ops.poisson_mg_transfer("restrict", shape, B, tables, b=cu(A["b"]), q=torch.zeros_like(x), c=ptr)
    out["Pe"], out["PTr"] = pe, ptr
    return out


def apply_axes32(a, shape, mats):
    """The float32 run of a transfer as the kernels state it: (B, n) float32 times per-axis float32 matrices (memory order), x first; per
    output the nonzero terms in index order, every product and every addition rounded to float32 (a BLAS product fuses or reorders
    them, which is another statement with another error)."""
    t = a.reshape(a.shape[0], *shape)
    for d in range(len(shape) - 1, -1, -1):
        m = mats[d]
        t = np.moveaxis(t, 1 + d, -1)
        out = np.zeros(t.shape[:-1] + (m.shape[0],), np.float32)
        for i in range(m.shape[0]):
            acc = np.zeros(t.shape[:-1], np.float32)
            for k in np.nonzero(m[i])[0]:
                acc = acc + m[i, k] * t[..., k]
            out[..., i] = acc
        t = np.moveaxis(out, -1, 1 + d)
    assert t.dtype == np.float32
    return np.ascontiguousarray(t).reshape(a.shape[0], -1)


@pytest.mark.parametrize("mask_batched", [False, True], ids=["shared-masks", "per-sample-masks"])
@pytest.mark.parametrize("sizes", TRANSFER_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_general_transfers_against_the_explicit_P(sizes, mask_batched):
    B = 3
    shape = tuple(sizes[::-1])                                # memory order
    cshape = tuple(s // 2 + 1 for s in shape)
    nf, nc = int(np.prod(shape)), int(np.prod(cshape))
    rng = np.random.default_rng(nf + int(mask_batched))
    A = {k: rng.standard_normal((B, nf)).astype(np.float32) for k in ("b", "q", "x")}
    A["c"] = rng.standard_normal((B, nc)).astype(np.float32)
    A["fmask"], A["cmask"] = rng.random((B, nf)) < 0.25, rng.random((B, nc)) < 0.25
    got = run_transfers(shape, B, A, mask_batched)
    P = gr.prolongation(shape, cshape)
    assert P.shape == (nf, nc)
    fm = A["fmask"] if mask_batched else np.repeat(A["fmask"][:1], B, 0)
    cm = A["cmask"] if mask_batched else np.repeat(A["cmask"][:1], B, 0)
    f64 = {k: v.astype(np.float64) for k, v in A.items() if v.dtype == np.float32}
    P1 = [gr.prolong_1d(f, c, rounded=True).astype(np.float32) for f, c in zip(shape, cshape)]
    PT1 = [m.T.copy() for m in P1]
    r32 = apply_axes32(A["b"] - A["q"], shape, PT1)
    e32_ = apply_axes32(A["c"], cshape, P1)
    ref64 = dict(restrict=np.where(cm, 0, (f64["b"] - f64["q"]) @ P), prolong=f64["x"] + np.where(fm, 0, f64["c"] @ P.T),
                 restrict_nomask=(f64["b"] - f64["q"]) @ P, prolong_nomask=f64["x"] + f64["c"] @ P.T, Pe=f64["c"] @ P.T, PTr=f64["b"] @ P)
    ref32 = dict(restrict=np.where(cm, np.float32(0), r32), prolong=A["x"] + np.where(fm, np.float32(0), e32_), restrict_nomask=r32,
                 prolong_nomask=A["x"] + e32_, Pe=e32_, PTr=apply_axes32(A["b"], shape, PT1))
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
    # Dirichlet nodes: exactly zero (restrict), bitwise untouched (prolong)
    assert not got["restrict"].cpu().numpy()[cm].any()
    assert np.array_equal(got["prolong"].cpu().numpy()[fm].view(np.int32), A["x"][fm].view(np.int32))
    # sample 2 alone: bitwise what it is in the batch
    A1 = {k: v[2:3] for k, v in A.items()}
    if not mask_batched:
        A1["fmask"], A1["cmask"] = A["fmask"][:1], A["cmask"][:1]
    solo = run_transfers(shape, 1, A1, mask_batched)
    for k in got:
        assert torch.equal(bits(solo[k][0]), bits(got[k][2])), k


def test_bad_transfer_arguments_are_refused_without_a_launch():
    from diffnet_amd import _lib, ops
    shape, B = (7, 16), 2                                     # 16 x 7 nodes
    tables = ops.MgTransferTables(shape, dev())
    nf, nc = 7 * 16, 4 * 9
    b, q, x = (torch.ones((B, nf), device=dev()) for _ in range(3))
    c = torch.full((B, nc), 5.0, device=dev())
    fn = _lib.lib().dn_poisson_mg_transfer
    stream = C.c_void_p(ops._raw_stream(dev()))

    def args(op):
        return ops.poisson_mg_transfer_args(op, shape, B, tables, **(dict(b=b, q=q, c=c) if op == "restrict" else dict(x=x, c=c)))

    for op in ("restrict", "prolong"):
        a, keep = args(op)
        a.coarse[0] = 8                                       # a wrong coarse extent
        assert fn(C.byref(a), stream) == -1
        a, keep = args(op)
        a.fine[1], a.coarse[1] = 3, 2                         # a general axis of 3 nodes
        assert fn(C.byref(a), stream) == -1
        for member in ("c", "b" if op == "restrict" else "x"):
            a, keep = args(op)
            setattr(a, member, getattr(a, member) + 4)        # a misaligned pointer
            assert fn(C.byref(a), stream) == -1
        a, keep = args(op)
        a.parents[0] += 8
        assert fn(C.byref(a), stream) == -1
    torch.cuda.synchronize()
    assert torch.all(c == 5.0) and torch.all(x == 1.0), "nothing was launched"
    with pytest.raises(ValueError):
        ops.poisson_mg_transfer("restrict", (7, 15), B, tables, b=b, q=q, c=c)


# ---------------------------------------------------------------------------------------------
# cases shared by the V-cycle and solve tests: the references are computed once
# ---------------------------------------------------------------------------------------------
class GenCase(MgCase):
    """An MgCase with the levels of mg_general_ref: float64 with the exact weights, and the same levels with the float32-rounded ones."""

    def levels(self, b, rounded=False):
        key = ("glevels", b if ((self.nu is not None and self.nu.shape[0] > 1) or any(m.shape[0] > 1 for m, _, _ in self.cond)) else 0)
        if key not in self._ref:
            fx = sr.fixed_nodes(int(np.prod(self.shp)), self.conditions(b))
            lv = gr.hierarchy(self.geom, self.pick(self.nu, b), fx, self.jac)
            self._ref[key] = (lv, gr.with_rounded_weights(lv))
        return self._ref[key][int(rounded)]

    def mg_reference(self, b, tol=1e-6):
        """(u64, x32, info32, err32, info64): the dense solution, the float32 PCG run (rounded weights) and its error, the float64 run's info."""
        key = ("gmgref", b, tol)
        if key not in self._ref:
            K, rhs = self.system(b)
            cond, x0 = self.conditions(b), self.pick(self.u0, b)
            u64 = sr.dense_solve(K, rhs, cond, x0)
            kw = dict(tol=tol, omega=omega_of(self.geom), maxiter=200)
            x32, i32 = gr.pcg(K, rhs, cond, x0, levels=self.levels(b, True), dtype=np.float32, **kw)
            _, i64 = gr.pcg(K, rhs, cond, x0, levels=self.levels(b), **kw)
            self._ref[key] = (u64, x32, i32, np.max(np.abs(x32 - u64)) / max(np.max(np.abs(u64)), 1e-300), i64)
        return self._ref[key]


def make_cases():
    cases = {}

    def add(name, sizes, B, seed, kind, form="box", ngp=2):
        c = GenCase(name, sizes, B, ngp, seed)
        c.f = 10 * c.rng.standard_normal((B, *c.shp))
        box = box_image(c.shp)[None]
        if kind == "box":                                    # box faces alone, nu absent
            c.cond = [(box, 0.0, form)]
        elif kind == "disk":                                 # box faces plus an immersed disk with a value (a mask image), shared nu
            c.nu = c.rng.uniform(0.5, 1.5, (1, *c.shp))
            c.cond = [(box, 0.0, form), (disk_image(c.shp)[None], 0.75, "f32")]
        else:                                                # random per-sample nu, a value field on the box, random u0
            c.nu = c.rng.uniform(0.5, 1.5, (B, *c.shp))
            c.u0 = c.rng.standard_normal((1, *c.shp))
            c.cond = [(box, c.rng.standard_normal((1, *c.shp)), form)]
        cases[name] = c

    for sizes in ((8, 8), (12, 7), (16, 16), (6, 7, 10)):
        tag = "x".join(map(str, sizes))
        add(tag + "-disk", sizes, 2, 302, "disk", "u8")
        add(tag + "-nu", sizes, 3, 303, "nu", "f32")
    add("16x16-box", (16, 16), 1, 301, "box")
    add("23x16-nu", (23, 16), 2, 304, "nu", "u8", ngp=3)
    add("8x8x8-disk", (8, 8, 8), 1, 306, "disk")
    add("17x17-nu", (17, 17), 2, 307, "nu", "f32")
    return cases


CASES = make_cases()
VCYCLE_NAMES = [n for n in CASES if n.split("-")[0] in ("8x8", "12x7", "16x16", "6x7x10") and not n.endswith("-box")]


# ---------------------------------------------------------------------------------------------
# b. one V-cycle
# ---------------------------------------------------------------------------------------------
OTHER_CYCLE = dict(mg_sweeps=2, mg_coarse_sweeps=1, mg_max_levels=2)
VCYCLES = [(n, {}) for n in VCYCLE_NAMES] + [(n, OTHER_CYCLE) for n in VCYCLE_NAMES if n.endswith("-nu")]


@pytest.mark.parametrize("name, options", VCYCLES, ids=[n + ("-2sweeps-2levels" if o else "") for n, o in VCYCLES])
def test_one_general_vcycle_against_the_restatement(name, options):
    from diffnet_amd import solve
    c = CASES[name]
    kw = c.torch_inputs()
    B = kw.pop("batch")
    s = solve.PoissonSolver(c.geom, B, **kw, **GENERAL, **options).setup()
    assert [L.shape for L in s.mg.levels] == gr.level_shapes(c.shp, options.get("mg_max_levels"))
    assert s.mg.levels[0].tables is not None, "the finest transfer of these meshes is a general one"
    rng = np.random.default_rng(5)
    r = rng.standard_normal((B, *c.shp))
    for b in range(B):
        r[b][sr.fixed_nodes(r[b].size, c.conditions(b)).reshape(c.shp)] = 0.0       # a CG residual is zero on the Dirichlet nodes
    r = r.astype(np.float32)
    z = s.apply_preconditioner(cu(r)[:, None])
    zc = solve.PoissonSolver(c.geom, B, **kw, **GENERAL, phases="composed", **options).setup().apply_preconditioner(cu(r)[:, None])
    mgkw = dict(sweeps=options.get("mg_sweeps", 1), omega=omega_of(c.geom), coarse_sweeps=options.get("mg_coarse_sweeps", 4))
    for b in range(B):
        nl = options.get("mg_max_levels")
        z64 = gr.vcycle(c.levels(b)[:nl], r[b].ravel(), **mgkw)
        z32 = gr.vcycle(c.levels(b, True)[:nl], r[b].ravel(), dtype=np.float32, **mgkw)
        assert z32.dtype == np.float32
        scale = np.max(np.abs(z64))
        e32 = np.max(np.abs(z32 - z64)) / scale
        for tag, t in (("fused", z), ("composed", zc)):
            got = t[b].double().cpu().numpy().ravel()
            e = np.max(np.abs(got - z64)) / scale
            print(f"V-cycle {name}[{b}] {tag}: error {e:.3e}, float32 reference {e32:.3e}, ratio {e / e32:.2f}")
            assert e <= MARGIN * e32, (tag, b)
            assert not got[c.levels(b)[0]["fixed"]].any(), "z is zero on the Dirichlet nodes"
    # the coarse Dirichlet images and coefficients are those of the restatement
    for l, L in enumerate(s.mg.levels):
        for b in range(B):
            ref = c.levels(b)[l]
            img = L.img[b if L.img.shape[0] > 1 else 0].cpu().numpy().ravel() != 0
            assert np.array_equal(img, ref["fixed"]), (l, b)


# ---------------------------------------------------------------------------------------------
# c. whole solves
# ---------------------------------------------------------------------------------------------
def gen_solve(c, samples=None, **options):
    from diffnet_amd import solve
    kw = c.torch_inputs(samples)
    kw.update(GENERAL)
    kw.update(options)
    return solve.poisson_solve(c.geom, **kw)


@pytest.mark.parametrize("name", ["16x16-nu", "23x16-nu", "8x8x8-disk"])
def test_general_multigrid_solve_against_the_dense_solution(name):
    from diffnet_amd import ops, solve
    c = CASES[name]
    kw = c.torch_inputs()
    s = solve.PoissonSolver(c.geom, tol=1e-6, **GENERAL, **kw)
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
        print(f"general multigrid solve {name}[{b}]: {info.iterations[b]} iterations (float32 reference {i32['iterations']}, float64 {i64['iterations']}), "
              f"error {err:.3e}, float32 reference {err32:.3e}, ratio {err / err32:.2f}")
        assert err <= MARGIN * err32
        K, rhs = c.system(b)
        fxn = sr.fixed_nodes(len(rhs), c.conditions(b))
        Rref = np.where(fxn, 0, K.astype(np.float32) @ x32.astype(np.float32) - rhs.astype(np.float32)).astype(np.float64)
        gap_ref = np.linalg.norm(Rref + i32["r"]) / np.sqrt(i32["rr0"])
        print(f"general multigrid solve {name}[{b}]: true residual against the recurrence |R + r| = {gaps[b]:.3e} |r0|, float32 reference {gap_ref:.3e}, ratio {gaps[b] / gap_ref:.2f}")
        assert gaps[b] <= MARGIN * gap_ref
        np.testing.assert_allclose(info.rr0[b], i32["rr0"], rtol=1e-4)


def test_general_multigrid_and_jacobi_reach_the_same_solution():
    from diffnet_amd import solve
    c = CASES["16x16-nu"]
    um, im = gen_solve(c, tol=1e-6)
    uj, ij = solve.poisson_solve(c.geom, tol=1e-6, precondition="jacobi", **c.torch_inputs())
    assert im.converged.all() and ij.converged.all()
    for b in range(c.B):
        u64, _, _, err32m, _ = c.mg_reference(b)
        _, _, _, err32j = c.reference(b)
        for tag, u, ref in (("multigrid", um, err32m), ("jacobi", uj, err32j)):
            err = np.max(np.abs(u[b].double().cpu().numpy().ravel() - u64)) / np.max(np.abs(u64))
            print(f"precondition {tag} [{b}]: error {err:.3e}, float32 reference {ref:.3e}, ratio {err / ref:.2f}")
            assert err <= MARGIN * ref
    print("iterations general multigrid", im.iterations, "jacobi", ij.iterations)
    assert np.all(im.iterations < ij.iterations)


def test_a_nested_mesh_solves_bitwise_the_same_under_both_rules():
    from diffnet_amd import solve
    c = CASES["17x17-nu"]
    ug, ig = gen_solve(c, tol=1e-6)
    un, i_n = solve.poisson_solve(c.geom, tol=1e-6, precondition="multigrid", **c.torch_inputs())
    assert ig.converged.all() and torch.equal(bits(ug), bits(un)) and np.array_equal(ig.iterations, i_n.iterations) and ig.rr.tobytes() == i_n.rr.tobytes()


@pytest.mark.parametrize("name", ["16x16-nu", "6x7x10-disk"])
def test_general_solve_is_bitwise_reproducible_and_batch_independent(name):
    c = CASES[name]
    u1, i1 = gen_solve(c, tol=1e-6)
    u2, i2 = gen_solve(c, tol=1e-6)
    assert i1.converged.all()
    assert torch.equal(bits(u1), bits(u2)) and np.array_equal(i1.iterations, i2.iterations) and i1.rr.tobytes() == i2.rr.tobytes()
    for b in range(c.B):
        us, is_ = gen_solve(c, [b], tol=1e-6)
        assert is_.iterations[0] == i1.iterations[b] and is_.rr[0:1].tobytes() == i1.rr[b:b + 1].tobytes(), (name, b)
        assert torch.equal(bits(us[0]), bits(u1[b])), (name, b)


def test_captured_general_iterations_replay_bitwise_and_setup_picks_up_nu():
    from diffnet_amd import solve
    c = CASES["16x16-nu"]
    kw = c.torch_inputs()
    kw.pop("batch")
    s = solve.PoissonSolver(c.geom, c.B, tol=1e-6, **GENERAL, **kw)
    s.setup().iterate(3)
    eager, st_e = s.solution.clone(), s.status()
    assert list(st_e.iterations) == [3] * c.B
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
    assert torch.equal(bits(s.solution), bits(eager)) and st_g.rr.tobytes() == st_e.rr.tobytes() and list(st_g.iterations) == [3] * c.B
    # an in-place change of nu reaches every level through setup()
    coarse_before = s.mg.levels[1].dinv.clone()
    kw["nu"].mul_(3.0)
    st = s.solve()
    fresh = solve.PoissonSolver(c.geom, c.B, tol=1e-6, **GENERAL, **{**kw, "nu": kw["nu"].clone()})
    st2 = fresh.solve()
    assert st.converged.all() and torch.equal(bits(s.solution), bits(fresh.solution)) and np.array_equal(st.iterations, st2.iterations)
    assert not torch.equal(s.mg.levels[1].dinv, coarse_before) and not torch.equal(s.solution, eager)


def test_all_three_mask_kinds_give_the_same_general_solve():
    from diffnet_amd import ops, solve
    c = CASES["16x16-box"]
    kw = c.torch_inputs()
    img = cu(box_image(c.shp)[None, None], torch.uint8)
    sols = {}
    for kind, mask in (("box", ops.BoxFaces("all")), ("packed", ops.PackedMask.pack(img)), ("u8", img), ("f32", img.float())):
        kw["dirichlet"] = [ops.Dirichlet(mask, 0.0)]
        sols[kind], info = solve.poisson_solve(c.geom, tol=1e-6, **GENERAL, **kw)
        assert info.converged.all(), kind
    u64, _, _, err32, _ = c.mg_reference(0)
    for kind, u in sols.items():
        err = np.max(np.abs(u[0].double().cpu().numpy().ravel() - u64)) / np.max(np.abs(u64))
        print(f"mask kind {kind}: error {err:.3e}, float32 reference {err32:.3e}, ratio {err / err32:.2f}")
        assert err <= MARGIN * err32


@pytest.mark.parametrize("name", ["12x7-disk", "6x7x10-nu"])
def test_composed_general_multigrid_agrees_with_fused(name):
    c = CASES[name]
    uf, i_f = gen_solve(c, tol=1e-6)
    uc, ic = gen_solve(c, tol=1e-6, phases="composed")
    assert i_f.converged.all() and ic.converged.all()
    print("iterations fused", i_f.iterations, "composed", ic.iterations)
    assert np.all(np.abs(i_f.iterations.astype(int) - ic.iterations.astype(int)) <= 1)
    for b in range(c.B):
        u64, _, _, err32, _ = c.mg_reference(b)
        for tag, u in (("fused", uf), ("composed", uc)):
            err = np.max(np.abs(u[b].double().cpu().numpy().ravel() - u64)) / np.max(np.abs(u64))
            print(f"{name}[{b}] {tag}: error {err:.3e}, float32 reference {err32:.3e}, ratio {err / err32:.2f}")
            assert err <= MARGIN * err32


def test_the_facades_forward_the_option():
    from diffnet_amd import DiffNet2DFEM, DiffNet3DFEM
    from diffnet_amd._lib import DiffNetHipError
    for cls, n, nsd in ((DiffNet2DFEM, 8, 2), (DiffNet3DFEM, 6, 3)):
        m = cls(None, domain_size=n, nsd=nsd)
        shp = (n,) * nsd
        f = torch.ones((1, 1, *shp), device=dev())
        dl = [(cu(box_image(shp)[None, None], torch.uint8), 0.0)]
        u, info = m.solve(f=f, dirichlet=dl, **GENERAL)
        uj, ij = m.solve(f=f, dirichlet=dl, tol=1e-6)
        assert info.converged.all() and torch.isfinite(u).all() and info.iterations[0] < 10
        assert float((u - uj).abs().max()) <= 1e-3 * float(uj.abs().max())
        with pytest.raises(DiffNetHipError, match="cannot be coarsened"):
            m.solve(f=f, dirichlet=dl, precondition="multigrid")


# ---------------------------------------------------------------------------------------------
# d. iteration counts: conditions, not timings
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 32, 64])
def test_general_iteration_count_against_the_float64_restatement(n):
    from diffnet_amd import ops, solve
    g, nu, f, ref_its = reference_count(n)
    dl = [ops.Dirichlet(ops.BoxFaces("all"), 0.0)]
    u, info = solve.poisson_solve(g, cu(nu)[None, None], cu(f)[None, None], dirichlet=dl, tol=1e-5, check_every=1, **GENERAL)
    print(f"{n}^2: {info.iterations[0]} iterations, float64 restatement {ref_its}")
    assert info.converged.all() and info.iterations[0] <= ref_its + 2      # 2: float32 rounding of alpha and beta
    if n == 64:
        uj, ij = solve.poisson_solve(g, cu(nu)[None, None], cu(f)[None, None], dirichlet=dl, tol=1e-5, check_every=1, precondition="jacobi")
        print(f"{n}^2: Jacobi {ij.iterations[0]} iterations")
        assert ij.converged.all() and info.iterations[0] < ij.iterations[0]
        assert ref_its <= reference_count(16)[3] + GROWTH_MARGIN


# ---------------------------------------------------------------------------------------------
# e. implicit gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(8, 8), (6, 6, 6)])
def test_implicit_gradients_with_general_multigrid_against_the_dense_derivative(sizes):
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
    u, info = solve.poisson_solve(geom, nu_t, f_t, dirichlet=dl, jac=jac, tol=tol, **GENERAL)
    assert info.converged.all() and u.requires_grad
    (u * cu(w)[:, None]).sum().backward()
    assert info.adjoint is not None and info.adjoint.converged.all(), "the adjoint solve goes through the same solver"
    g64, g32 = [np.zeros_like(nu), np.zeros_like(f)], [np.zeros_like(nu), np.zeros_like(f)]
    cond, hom = [(box, val[0])], [(box, 0.0)]
    om = omega_of(geom)
    for b in range(B):
        K, rhs = sr.dense_system(geom, nu[b], f[b], None, jac)
        lv = gr.with_rounded_weights(gr.hierarchy(geom, nu[b], box, jac))
        u64, lam64 = sr.dense_solve(K, rhs, cond), sr.dense_adjoint(K, w[b], cond)
        x32, i32 = gr.pcg(K, rhs, cond, levels=lv, tol=tol, dtype=np.float32, omega=om)
        l32, j32 = gr.pcg(K, np.zeros_like(rhs), hom, levels=lv, tol=tol, dtype=np.float32, extra_load=w[b].ravel(), omega=om)
        assert i32["converged"] and j32["converged"]
        for dst, (uu, ll) in ((g64, (u64, lam64)), (g32, (x32, l32))):
            gn, gf = sr.implicit_grads(geom, uu, ll, jac)
            dst[0][b] += gn
            dst[1][b] += gf
    for k, (tag, got) in enumerate((("nu", nu_t.grad), ("f", f_t.grad))):
        got = got[:, 0].double().cpu().numpy()
        scale = np.max(np.abs(g64[k]))
        err, ref = np.max(np.abs(got - g64[k])) / scale, np.max(np.abs(g32[k] - g64[k])) / scale
        print(f"general multigrid gradient d/d{tag} {sizes}: error {err:.3e}, float32 reference {ref:.3e}, ratio {err / ref:.2f}")
        assert err <= MARGIN * ref
