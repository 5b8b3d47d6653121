"""Batched matrix-free conjugate-gradient solve of the discrete Q1 Poisson problem  Z (K_nu u~ - F f) = 0  -- the field the energy and
residual losses of this library converge to -- and its implicit derivative with respect to the nodal coefficient and forcing.

One iteration is the fused operator (q = Z K_nu p through a prepared `ops.PoissonPlan`) followed by the three vector phases of
`dn_poisson_cg` (include/diffnet_hip.h): per-sample dot products become per-sample alpha / beta on the device, converged samples of a
batch stand still, and nothing of an iteration touches the host but the launches themselves: a chunk of iterations can be captured
with torch.cuda.graph.

precondition="multigrid" replaces the diagonal by one geometric multigrid V-cycle per iteration (`_Multigrid` below): the levels are the
same operator rediscretised on nested meshes of halved element counts (`multigrid_levels`), each a prepared `ops.PoissonPlan` and a
`dn_poisson_diag`; the transfers and the damped-Jacobi update are `dn_poisson_mg`, and because z = M r now comes from memory the vector
phases are those of `dn_poisson_pcg`.  mg_coarsening="general" coarsens meshes that are not nested as well (an axis of e elements keeps
ceil(e / 2) over the same length); on a level with such an axis the transfers are `dn_poisson_mg_transfer`, which reads the per-axis
interpolation weights from small tables built here on the host.  The iteration count becomes roughly independent of the mesh; one iteration costs several
operator launches per level (DESIGN.md section 6 and profiles/poisson_multigrid.txt say where that pays).

Limits, stated plainly: Q1 meshes only (degree 1, rules of 2 to 4 points); Jacobi, multigrid or no preconditioning; multigrid by default
on nested meshes only (node counts k 2^(L-1) + 1 per axis with L >= 2), with mg_coarsening="general" on any mesh with at least 3 elements
per axis; a point smoother, so strongly anisotropic spacings or coefficient jumps that the coarse meshes cannot see still cost iterations.  Float32 CG stalls at a relative residual that
grows with the condition number of the mesh (README.md quotes measured levels); ask for a `tol` it can reach.
"""
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import DiffNetHipError
from .fem import FemGeometry
from .ops import Dirichlet, PackedMask


def _check_geom(geom):
    if geom.deg != 1:
        raise DiffNetHipError(f"PoissonSolver: Q1 meshes only (fem_basis_deg = 1), got degree {geom.deg}: the CG kernels and the "
                              "Jacobi diagonal are written for the Q1 operator")
    if not 2 <= geom.ngp_1d <= 4:
        raise DiffNetHipError(f"PoissonSolver: rules of 2 to 4 points per axis, got {geom.ngp_1d}")


def _check_coarsening(coarsening):
    if coarsening not in ("nested", "general"):
        raise ValueError('mg_coarsening must be "nested" or "general"')


def multigrid_levels(geom, max_levels=None, coarsening="nested"):
    """[(node_shape, hs), ...] of the multigrid levels of a mesh, fine first: node_shape in memory order (as geom.node_shape), hs the
    spacings (as geom.hs).  coarsening="nested": a level is coarsened -- element counts halved, spacings doubled -- while every axis has
    an even element count and the coarse mesh keeps at least 2 elements per axis.  "general": while every axis has at least 3 elements;
    an axis of e elements keeps ceil(e / 2) over the same length (spacing h e / ceil(e / 2)), so an axis with an even count is coarsened
    exactly as under "nested" and an odd one loses its nesting on that level alone.  At most `max_levels` levels.  Pure: needs no GPU."""
    _check_coarsening(coarsening)
    if max_levels is not None and int(max_levels) < 1:
        raise ValueError("mg_max_levels must be at least 1")
    levels = [(tuple(geom.node_shape), tuple(geom.hs))]
    while max_levels is None or len(levels) < int(max_levels):
        shape, hs = levels[-1]
        nel = [s - 1 for s in shape]
        if coarsening == "general":
            if any(e < 3 for e in nel):
                break
            # hs is in the order x, y[, z], the shape in memory order; e / ceil(e / 2) is exactly 2.0 for an even e
            levels.append((tuple((e + 1) // 2 + 1 for e in nel), tuple(h * (e / ((e + 1) // 2)) for h, e in zip(hs, nel[::-1]))))
            continue
        if any(e % 2 or e // 2 < 2 for e in nel):
            break
        levels.append((tuple(e // 2 + 1 for e in nel), tuple(2.0 * h for h in hs)))
    return levels


def _level_geometry(geom, shape, hs):
    return FemGeometry(geom.nsd, shape[::-1], hs, geom.deg, geom.ngp_1d, geom.gpx_1d, geom.gpw_1d)


def _multigrid_levels_or_raise(geom, max_levels, coarsening="nested"):
    levels = multigrid_levels(geom, max_levels, coarsening)
    if len(levels) < 2 and coarsening == "general":
        raise DiffNetHipError(f'precondition="multigrid": the mesh of {"x".join(map(str, geom.node_shape))} nodes cannot be coarsened (mg_coarsening="general" '
                              "needs at least 3 elements on every axis, and mg_max_levels at least 2).  Under the default "
                              'mg_coarsening="nested" the node counts that work are k 2^(L-1) + 1 per axis; or use precondition="jacobi"')
    if len(levels) < 2:
        raise DiffNetHipError(f'precondition="multigrid": the mesh of {"x".join(map(str, geom.node_shape))} nodes cannot be coarsened (every axis needs an '
                              'even element count and 2 elements left on the coarse mesh under mg_coarsening="nested").  Node counts that work: '
                              'k 2^(L-1) + 1 per axis with k >= 2 and L >= 2 levels, e.g. 129, 257, 385, 513; mg_coarsening="general" coarsens any '
                              'mesh with at least 3 elements per axis; or use precondition="jacobi"')
    return levels


def element_lambda_max(geom):
    """lambda_max(D_e^-1 K_e) of one element of the mesh with nu = 1, in float64: an upper bound of lambda_max(D^-1 K) of the assembled
    constant-coefficient operator (1.5 for square and cubic elements, up to 3 / 4 for stretched ones in 2-D / 3-D) that a variable nu
    moves by a few per cent (DESIGN.md section 6 lists measured values)."""
    B = np.asarray(geom.basis, np.float64)[:, :2]
    D = np.asarray(geom.dbasis, np.float64)[:, :2]
    w = np.asarray(geom.gpw_1d, np.float64)
    M1 = np.einsum("g,ga,gc->ac", w, B, B)
    K = 0.0
    for d in range(geom.nsd):
        term = np.ones((1, 1))
        for ax in range(geom.nsd):
            term = np.kron(term, np.einsum("g,ga,gc->ac", w, D, D) * (2.0 / geom.hs[d]) ** 2 if ax == d else M1)
        K = K + term
    dg = np.diag(K)
    return float(np.linalg.eigvalsh(K / np.sqrt(np.outer(dg, dg)))[-1])


def default_mg_omega(geom):
    """The damping of the Jacobi smoother when mg_omega is None: (4 / 3) / element_lambda_max -- 8 / 9 on square and cubic elements --
    so that omega lambda_max(D^-1 K) stays near 4 / 3, well inside the < 2 that keeps the V-cycle positive definite."""
    return (4.0 / 3.0) / element_lambda_max(geom)


def _tensors_of(nu, f, f_gp, u0, dl, load=None):
    ts = [nu, f.tensor if isinstance(f, ops.LoadVector) else f, f_gp, u0, load]
    for d in dl:
        ts += [d.mask if isinstance(d.mask, torch.Tensor) else getattr(d.mask, "bits", None), d.value]
    return [t for t in ts if isinstance(t, torch.Tensor)]


class PoissonSolver:
    """Preconditioned CG on FIXED buffers for `batch` samples of one mesh.

        solver = PoissonSolver(geom, batch, nu=None, f=None, f_gp=None, dirichlet=(), u0=None, jac=1.0, tol=1e-5, atol=0.0,
                               maxiter=None, check_every=None, precondition="jacobi", mg_sweeps=1, mg_omega=None,
                               mg_coarse_sweeps=4, mg_max_levels=None, mg_coarsening="nested")
        solver.setup()        # diagonal + initial residual + INIT; call again after changing nu / f / masks / u0 in place
        solver.iterate(k)     # k iterations: no allocation, no device-to-host copy, no synchronisation (capturable)
        solver.status()       # one synchronising read of the per-sample scalars
        solver.solution       # (B,1,*N), the Dirichlet values on the Dirichlet nodes

    nu, f: contiguous float32 nodal fields (B|1,1,*N) or None; f_gp (B|1,G,*nel) instead of f.  dirichlet: up to two conditions,
    `Dirichlet(mask, value)` or (mask, value) with mask a float32 / uint8 image, a `PackedMask` or `BoxFaces`, value a constant or a
    nodal field.  The operator launches take the conditions in whatever form they accept for the mesh; the diagonal reads images.
    The tensors are read in place by every launch (as with `ops.PoissonPlan`): they must be usable as they are.
    u0: the initial guess (B|1,1,*N), zero when None.  tol: relative residual |r| / |r0| at which a sample stops; atol: absolute |r|.
    maxiter: 20 * max(node_shape) when None -- a heuristic for coefficient contrast near 1 (Jacobi-CG needs O(n) iterations on an
    n-node-wide mesh); `poisson_solve` stops there.  precondition: "jacobi", None (dinv = 1 on the free nodes) or "multigrid": one
    V-cycle per iteration with mg_sweeps damped-Jacobi sweeps before and after each coarse correction (equal, so that M stays symmetric),
    damping mg_omega (None: `default_mg_omega(geom)`), mg_coarse_sweeps sweeps on the coarsest level, at most mg_max_levels levels; a mesh
    that `multigrid_levels` cannot coarsen raises DiffNetHipError; mg_coarsening: "nested" (node counts k 2^(L-1) + 1 per axis) or "general"
    (any mesh with at least 3 elements per axis: `multigrid_levels`, `_Multigrid`).  check_every: iterations between the status reads of `solve()`, 32
    when None (2 with "multigrid", whose iterations are few and dear).
    load: an ASSEMBLED right-hand side (B,1,*N) added to F f (read as zero on the Dirichlet nodes): what the adjoint solve needs.
    phases: "fused" (the dn_poisson_cg kernels) or "composed" (the same recurrences from torch ops on `ops.residual`: a measuring
    stick, about a dozen launches per iteration)."""

    def __init__(self, geom, batch, nu=None, f=None, f_gp=None, dirichlet=(), u0=None, jac=1.0, tol=1e-5, atol=0.0, maxiter=None,
                 check_every=None, precondition="jacobi", load=None, phases="fused", device=None, mg_sweeps=1, mg_omega=None,
                 mg_coarse_sweeps=4, mg_max_levels=None, mg_coarsening="nested"):
        _check_geom(geom)
        _check_coarsening(mg_coarsening)
        if precondition not in ("jacobi", "multigrid", None):
            raise ValueError('precondition must be "jacobi", "multigrid" or None')
        if precondition == "multigrid":
            if int(mg_sweeps) < 1 or int(mg_coarse_sweeps) < 1:
                raise ValueError("mg_sweeps and mg_coarse_sweeps must be at least 1")
            mg_levels = _multigrid_levels_or_raise(geom, mg_max_levels, mg_coarsening)
        if phases not in ("fused", "composed"):
            raise ValueError('phases must be "fused" or "composed"')
        self.geom, self.B = geom, int(batch)
        self.dl = ops._norm_dirichlet(dirichlet)
        self.nu, self.f, self.f_gp, self.u0, self.load = nu, f, f_gp, u0, load
        for t in _tensors_of(nu, f, f_gp, u0, self.dl, load):
            if t.requires_grad:
                raise DiffNetHipError("PoissonSolver works outside autograd: detach its inputs (poisson_solve differentiates the solve)")
        if device is None:
            ts = [t for t in _tensors_of(nu, f, f_gp, u0, self.dl, load) if t.is_cuda]
            device = ts[0].device if ts else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.jac, self.tol, self.atol = float(jac), float(tol), float(atol)
        self.maxiter = int(maxiter) if maxiter is not None else 20 * max(geom.node_shape)
        # iterations between two status() reads of solve(): a read costs about one multigrid iteration on a small mesh and every iteration past
        # convergence still runs its operator launches and V-cycle on the batch, so multigrid looks often
        self.check_every = max(1, int(check_every)) if check_every is not None else (2 if precondition == "multigrid" else 32)
        self.precondition, self.phases = precondition, phases
        shape = (self.B, 1, *geom.node_shape)
        self.n = int(np.prod(geom.node_shape))
        new = lambda: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.x, self.r, self.p, self.q, self.dinv = new(), new(), new(), new(), new()
        self.homog = [Dirichlet(d.mask, 0.0) for d in self.dl]
        # the two operator launches on fixed buffers: out = Z (K x~ - F f) into q (setup), q = Z K p (every iteration)
        self._plan0 = ops.PoissonPlan(geom, self.x, nu, f, f_gp, self.dl, alpha=1.0, beta=1.0, c=0.0, wscale=self.jac, want_out=True,
                                      want_sums=False, out=self.q)
        self._plan = ops.PoissonPlan(geom, self.p, nu, None, None, self.homog, alpha=1.0, beta=0.0, c=0.0, wscale=self.jac, want_out=True,
                                     want_sums=False, out=self.q)
        self.mg = None
        if precondition == "multigrid":
            self.z = new()
            self.mg = _Multigrid(self, mg_levels, int(mg_sweeps), default_mg_omega(geom) if mg_omega is None else float(mg_omega), int(mg_coarse_sweeps))
        if phases == "fused":
            self.state = ops.poisson_cg_state(self.B, self.device)
            self.workspace = ops.poisson_cg_workspace(self.n, self.B, self.device)
            mk = lambda ph: ops.poisson_cg_args(ph, self.x, self.r, self.p, self.q, self.dinv, self.state, self.workspace, self.tol, self.atol)
            self._args = {ph: mk(ph) for ph in ("init", "dot", "update", "direction")}
            fn = _lib.lib().dn_poisson_cg
            refs = [ops.C.byref(self._args[ph][0]) for ph in ("dot", "update", "direction")]
            self._fn, self._refs = fn, refs
            if self.mg is not None:
                # z = M r comes from memory: the phases of dn_poisson_pcg around the V-cycle, DOT unchanged
                pk = lambda ph: ops.poisson_pcg_args(ph, self.x, self.r, self.p, self.q, self.z, self.state, self.workspace, self.tol, self.atol)
                self._pargs = {ph: pk(ph) for ph in ("resid0", "update", "rz", "direction")}
                self._pfn = _lib.lib().dn_poisson_pcg
                self._prefs = {ph: ops.C.byref(a[0]) for ph, a in self._pargs.items()}
        self._ready = False

    # -- setup -------------------------------------------------------------------------------------------------------------------
    def _fixed(self):
        """bool image of the Dirichlet nodes (broadcastable to x), None without conditions."""
        fx = None
        for d in self.dl:
            c = ops._dirichlet_cond(ops._mask_image(d.mask, self.x))
            fx = c if fx is None else fx | c
        return fx

    def setup(self):
        with torch.no_grad():
            if self.u0 is None:
                self.x.zero_()
            else:
                self.x.copy_(self.u0.to(self.device).expand_as(self.x))
            if self.dl:
                self.x.copy_(ops._apply_dirichlet(self.x, self.dl))
            ops.poisson_diag(self.geom, self.B, self.nu, self.dl, wscale=self.jac, unit=self.precondition is None, out=self.dinv)
            if self.mg is not None:
                self.mg.setup()
            self._plan0.launch()
            if self.load is not None:
                fx = self._fixed()
                ld = self.load.to(self.device).expand_as(self.q)
                self.q.sub_(ld if fx is None else torch.where(fx, torch.zeros_like(ld), ld))
            if self.phases == "composed":
                self._composed_init()
            elif self.mg is None:
                ops.poisson_cg_launch(self._args["init"][0], self.device)
            else:
                s = ops.C.c_void_p(ops._raw_stream(self.device))
                self._pcg("resid0", s)
                self._precondition_and_direct(s)
        self._ready = True
        return self

    # -- iterations --------------------------------------------------------------------------------------------------------------
    def iterate(self, k=1):
        if not self._ready:
            raise DiffNetHipError("PoissonSolver.iterate: call setup() first")
        if self.phases == "composed":
            with torch.no_grad():
                for _ in range(int(k)):
                    self._composed_iteration()
            return self
        plan, fn, refs = self._plan, self._fn, self._refs
        s = ops.C.c_void_p(ops._raw_stream(self.device))
        if self.mg is not None:
            for _ in range(int(k)):
                plan.launch()
                rc = fn(refs[0], s)               # DOT
                if rc:
                    _lib.check(rc, "dn_poisson_cg")
                self._pcg("update", s)
                self._precondition_and_direct(s)
            return self
        for _ in range(int(k)):
            plan.launch()
            for ref in refs:
                rc = fn(ref, s)
                if rc:
                    _lib.check(rc, "dn_poisson_cg")
        return self

    def _pcg(self, phase, s):
        rc = self._pfn(self._prefs[phase], s)
        if rc:
            _lib.check(rc, "dn_poisson_pcg")

    def _precondition_and_direct(self, s):
        """z = M r (one V-cycle), rz and beta, p = z + beta p."""
        self.mg.launch(s)
        self._pcg("rz", s)
        self._pcg("direction", s)

    def apply_preconditioner(self, r):
        """z = M r for a (B,1,*N) float32 field r, as a new tensor: dinv r, or one V-cycle.  For inspection and tests; needs setup() and
        (with "multigrid") overwrites the solver's r, z and q -- call setup() again before iterating."""
        if not self._ready:
            raise DiffNetHipError("PoissonSolver.apply_preconditioner: call setup() first")
        with torch.no_grad():
            r = r.to(self.device, torch.float32).expand_as(self.x)
            if self.mg is None:
                return self.dinv * r
            if self.phases == "composed":
                return self.mg.composed(r.contiguous())
            self.r.copy_(r)
            self.mg.launch(ops.C.c_void_p(ops._raw_stream(self.device)))
            return self.z.clone()

    def status(self):
        """Per-sample scalars after one synchronising read: iterations (int32), rel_residual = sqrt(rr / rr0), converged, breakdown,
        active (numpy arrays of B) and rr, rr0."""
        if not self._ready:
            raise DiffNetHipError("PoissonSolver.status: call setup() first")
        if self.phases == "fused":
            st = ops.poisson_cg_read_state(self.state)
            rr, rr0, active, its, flags = st["rr"].copy(), st["rr0"].copy(), st["active"] != 0, st["iterations"].copy(), st["flags"].copy()
        else:
            c = self._c
            rr, rr0, active, its, flags = (c[k].cpu().numpy() for k in ("rr", "rr0", "active", "iterations", "flags"))
            active = active != 0
        thr = np.maximum(np.float64(np.float32(self.tol)) ** 2 * rr0, np.float64(np.float32(self.atol)) ** 2)
        breakdown = (flags & _lib.CG_BREAKDOWN) != 0
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(rr0 > 0, np.sqrt(rr / np.where(rr0 > 0, rr0, 1.0)), 0.0)
        return types.SimpleNamespace(iterations=its.astype(np.int32), rel_residual=rel, converged=~active & ~breakdown & (rr <= thr),
                                     breakdown=breakdown, active=active, rr=rr, rr0=rr0)

    @property
    def solution(self):
        return self.x

    def solve(self):
        """setup(), then iterate(check_every) / status() until no sample is active or maxiter is reached.  Returns status()."""
        self.setup()
        done = 0
        st = self.status()
        while st.active.any() and done < self.maxiter:
            k = min(self.check_every, self.maxiter - done)
            self.iterate(k)
            done += k
            st = self.status()
        st.maxiter = self.maxiter
        return st

    # -- the same recurrences from torch ops (phases="composed") -------------------------------------------------------------------
    def _dots(self, a, b):
        return (a.double() * b.double()).flatten(1).sum(1)

    def _composed_precondition(self, r):
        return self.dinv * r if self.mg is None else self.mg.composed(r)

    def _composed_init(self):
        r = -self.q
        self.r.copy_(r)
        self.p.copy_(self._composed_precondition(r))
        rr = self._dots(r, r)
        at = float(np.float32(self.atol)) ** 2
        z = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._c = dict(rz=self._dots(r, self.p), rr=rr, rr0=rr.clone(), active=(rr > at).to(torch.int32), iterations=z.clone(), flags=z.clone())

    def _composed_iteration(self):
        c = self._c
        col = lambda v: v.reshape((-1, 1) + (1,) * self.geom.nsd)
        q = ops.residual(self.geom, self.p, self.nu, None, None, self.homog, self.jac)
        act = c["active"] != 0
        pq = self._dots(self.p, q)
        ok = act & (pq > 0)
        c["flags"] = c["flags"] | (act & ~ok).to(torch.int32)
        alpha = torch.where(ok, c["rz"] / torch.where(ok, pq, torch.ones_like(pq)), torch.zeros_like(pq)).float()
        okc = col(ok)
        x = torch.where(okc, torch.addcmul(self.x, col(alpha), self.p), self.x)
        r = torch.where(okc, torch.addcmul(self.r, col(-alpha), q), self.r)
        z = self._composed_precondition(r)
        rzn, rr = self._dots(r, z), self._dots(r, r)
        beta = torch.where(ok, rzn / torch.where(ok, c["rz"], torch.ones_like(pq)), torch.zeros_like(pq)).float()
        thr = torch.clamp(float(np.float32(self.tol)) ** 2 * c["rr0"], min=float(np.float32(self.atol)) ** 2)
        c["rz"] = torch.where(ok, rzn, c["rz"])
        c["rr"] = torch.where(ok, rr, c["rr"])
        c["iterations"] = c["iterations"] + ok.to(torch.int32)
        still = ok & (rr > thr)
        c["active"] = still.to(torch.int32)
        self.x.copy_(x)
        self.r.copy_(r)
        self.p.copy_(torch.where(col(still), torch.addcmul(z, col(beta), self.p), self.p))


class _Multigrid:
    """The V-cycle z = M r of a PoissonSolver on FIXED buffers.  Level l is the same operator rediscretised: a FemGeometry with the same
    rule, element counts halved and spacings doubled l times, wscale = jac 2^(nsd l) (for a constant coefficient that IS the Galerkin
    product P^T K P), nu injected (every second node; a shared field stays shared, None stays None), the Dirichlet nodes the injection of
    the union of the fine conditions (one uint8 image per level, shared unless a mask is per sample; the values are homogeneous), dinv
    from dn_poisson_diag.  Under mg_coarsening="general" a level's shape and spacings are those of `multigrid_levels`, wscale =
    jac prod(hs_l / hs_0), and below a level with an axis of odd element count (`L.tables` is set: the per-axis float32 weights of
    `ops.MgTransferTables`, read by dn_poisson_mg_transfer and, as dense 1-D matrices, by the composed route) nu is interpolated
    multilinearly at the coarse nodes and a coarse node is a Dirichlet node where its nearest fine node is one -- both are injection on
    an axis that is nested; levels whose axes are all nested keep the dn_poisson_mg transfers.  Level 0 works on the solver's own r (right-hand side), z (the result), q and dinv.  Everything is prepared here;
    `launch` only launches; `setup` rebuilds what depends on nu and the masks."""

    def __init__(self, solver, levels, sweeps, omega, coarse_sweeps):
        s = self.solver = solver
        geom, B, dev = s.geom, s.B, s.device
        self.sweeps, self.omega, self.coarse_sweeps = sweeps, omega, coarse_sweeps
        if not omega > 0:
            raise ValueError("mg_omega must be positive")
        nb = 1                                              # batch extent of the Dirichlet images
        for d in s.dl:
            m = d.mask
            nb = max(nb, 1 if isinstance(m, ops.BoxFaces) else int(m.shape[0]))
        self.levels = []
        for l, (shape, hs) in enumerate(levels):
            g = geom if l == 0 else _level_geometry(geom, shape, hs)
            new = lambda: torch.zeros((B, 1, *shape), dtype=torch.float32, device=dev)
            # the level's own Jacobian over the fine one: 2^(nsd l), exactly, while every coarsening so far was nested
            L = types.SimpleNamespace(geom=g, shape=shape, wscale=s.jac * float(np.prod([hl / h0 for hl, h0 in zip(hs, geom.hs)])))
            # the transfers to the next level: dn_poisson_mg while every axis is nested, else dn_poisson_mg_transfer and its tables
            L.tables = None
            if l + 1 < len(levels) and any((n - 1) % 2 for n in shape):
                L.tables = ops.MgTransferTables(shape, dev)
                assert L.tables.coarse_shape == tuple(levels[l + 1][0])
            L.x, L.b, L.q, L.dinv = (s.z, s.r, s.q, s.dinv) if l == 0 else (new(), new(), new(), new())
            L.img = torch.zeros((nb, 1, *shape), dtype=torch.uint8, device=dev) if s.dl else None
            L.nu = s.nu if l == 0 or s.nu is None else torch.zeros((s.nu.shape[0], 1, *shape), dtype=torch.float32, device=dev)
            L.dl = s.homog if l == 0 else ([Dirichlet(L.img, 0.0)] if s.dl else [])
            L.plan = ops.PoissonPlan(g, L.x, L.nu, None, None, L.dl, alpha=1.0, beta=0.0, c=0.0, wscale=L.wscale, want_out=True,
                                     want_sums=False, out=L.q)
            self.levels.append(L)
        self._fn, self._tfn = _lib.lib().dn_poisson_mg, _lib.lib().dn_poisson_mg_transfer
        self._keep, self._seq = [], []
        self._build(0)
        k1 = torch.tensor([0.5, 1.0, 0.5], device=dev)                 # the composed cycle's transfers: P^T as a stride-2 convolution
        k2 = k1[:, None] * k1[None, :]
        self._stencil = (k2 if geom.nsd == 2 else k1[:, None, None] * k2[None])[None, None]

    def _mg(self, op, l, **arrays):
        L = self.levels[l]
        a, keep = ops.poisson_mg_args(op, L.shape, self.solver.B, omega=self.omega, **arrays)
        self._keep.append((a, keep))
        self._seq.append((1, ops.C.byref(a)))

    def _transfer(self, op, l, **arrays):
        """RESTRICT from / PROLONG onto level l: the nested kernels, or the general ones where an axis of the level is not nested."""
        L = self.levels[l]
        if L.tables is None:
            return self._mg(op, l, **arrays)
        a, keep = ops.poisson_mg_transfer_args(op, L.shape, self.solver.B, L.tables, **arrays)
        self._keep.append((a, keep))
        self._seq.append((2, ops.C.byref(a)))

    def _build(self, l):
        """The launches of level l and below, in order."""
        L, last = self.levels[l], l + 1 == len(self.levels)
        sweep = lambda: (self._seq.append((0, L.plan)), self._mg("smooth", l, x=L.x, b=L.b, q=L.q, dinv=L.dinv))
        self._mg("smooth0", l, x=L.x, b=L.b, dinv=L.dinv)
        for _ in range((self.coarse_sweeps if last else self.sweeps) - 1):
            sweep()
        if last:
            return
        C = self.levels[l + 1]
        self._seq.append((0, L.plan))
        self._transfer("restrict", l, b=L.b, q=L.q, c=C.b, mask=C.img)
        self._build(l + 1)
        self._transfer("prolong", l, x=L.x, c=C.x, mask=L.img)
        for _ in range(self.sweeps):
            sweep()

    def setup(self):
        s = self.solver
        every_second = (slice(None), slice(None)) + (slice(None, None, 2),) * s.geom.nsd
        for l, L in enumerate(self.levels):
            if L.img is not None:
                if l == 0:
                    fx = s._fixed()
                    L.img.copy_(fx.to(torch.uint8).expand_as(L.img))
                elif self.levels[l - 1].tables is None:
                    L.img.copy_(self.levels[l - 1].img[every_second])
                else:
                    L.img.copy_(self._coarse_image(self.levels[l - 1].img, L.shape))
            if l > 0:
                if L.nu is not None and self.levels[l - 1].tables is None:
                    L.nu.copy_(self.levels[l - 1].nu[every_second])
                elif L.nu is not None:
                    L.nu.copy_(self._coarse_field(self.levels[l - 1].nu, L.shape))
                ops.poisson_diag(L.geom, s.B, L.nu, L.dl, wscale=L.wscale, out=L.dinv)

    @staticmethod
    def _coarse_image(img, coarse_shape):
        """The Dirichlet image of the next level: on each axis the fine node nearest to the coarse node (the lower one of a tie) --
        injection on a nested axis, and faces map to faces."""
        for d, nc in enumerate(coarse_shape):
            nf = img.shape[2 + d]
            j = torch.arange(nc, device=img.device)
            img = img.index_select(2 + d, (2 * j * (nf - 1) + (nc - 1)) // (2 * (nc - 1)))
        return img

    @staticmethod
    def _coarse_field(nu, coarse_shape):
        """A nodal coefficient interpolated multilinearly at the nodes of the next level (`ops.mg_axis_interpolation` from the fine to
        the coarse mesh): injection on a nested axis."""
        for d, nc in enumerate(coarse_shape):
            j, w = ops.mg_axis_interpolation(nu.shape[2 + d], nc)
            j, w = torch.from_numpy(j).to(nu.device), torch.from_numpy(w).to(nu.device)
            bshape = [1] * nu.dim()
            bshape[2 + d] = nc
            nu = w[:, 0].reshape(bshape) * nu.index_select(2 + d, j) + w[:, 1].reshape(bshape) * nu.index_select(2 + d, j + 1)
        return nu

    def launch(self, stream):
        fn, tfn = self._fn, self._tfn
        for kind, what in self._seq:
            if kind == 0:
                what.launch()
            elif kind == 1:
                rc = fn(what, stream)
                if rc:
                    _lib.check(rc, "dn_poisson_mg")
            else:
                rc = tfn(what, stream)
                if rc:
                    _lib.check(rc, "dn_poisson_mg_transfer")

    # -- the same cycle from torch ops (phases="composed"): the measuring stick -------------------------------------------------------
    def composed(self, r, l=0):
        L, last = self.levels[l], l + 1 == len(self.levels)
        s = self.solver
        free = 1.0 if L.img is None else (L.img == 0).to(torch.float32)
        conv, convT = (F.conv2d, F.conv_transpose2d) if s.geom.nsd == 2 else (F.conv3d, F.conv_transpose3d)
        op = lambda x: ops.residual(L.geom, x, L.nu, None, None, L.dl, L.wscale)
        wd = self.omega * L.dinv
        x = wd * r
        for _ in range((self.coarse_sweeps if last else self.sweeps) - 1):
            x = x + wd * (r - op(x))
        if last:
            return x
        C = self.levels[l + 1]
        cfree = 1.0 if C.img is None else (C.img == 0).to(torch.float32)
        if L.tables is None:
            bc = cfree * conv(r - op(x), self._stencil, stride=2, padding=1)
            x = x + free * convT(self.composed(bc, l + 1), self._stencil, stride=2, padding=1)
        else:
            # a level that is not nested: the dense 1-D matrices of the kernels' own float32 tables, axis by axis
            def along_axes(t, transpose):
                for d, P in enumerate(L.tables.matrices):
                    t = torch.movedim(torch.tensordot(t, P, dims=([2 + d], [0 if transpose else 1])), -1, 2 + d)
                return t
            bc = cfree * along_axes(r - op(x), True)
            x = x + free * along_axes(self.composed(bc, l + 1), False)
        for _ in range(self.sweeps):
            x = x + wd * (r - op(x))
        return x


def _infer_batch(geom, batch, nu, f, f_gp, u0, dl):
    if batch is not None:
        return int(batch)
    B = 1
    for t in _tensors_of(nu, f, f_gp, u0, dl):
        if t.dim() == geom.nsd + 2:
            B = max(B, int(t.shape[0]))
    for d in dl:
        if isinstance(d.mask, PackedMask):
            B = max(B, int(d.mask.shape[0]))
    return B


def _plain(t):
    """A tensor as the prepared launches want it: detached, float32, contiguous (a copy only where needed)."""
    if isinstance(t, ops.LoadVector) or not isinstance(t, torch.Tensor):
        return t
    return t.detach().to(torch.float32).contiguous()


def _plain_conditions(dl):
    out = []
    for d in dl:
        m = d.mask
        if isinstance(m, torch.Tensor):
            m = (m.to(torch.uint8) if m.dtype == torch.bool else m).contiguous()
        out.append(Dirichlet(m, _plain(d.value)))
    return out


def _solve_plain(geom, B, nu, f, f_gp, dl, u0, load, opts):
    solver = PoissonSolver(geom, B, _plain(nu), _plain(f), _plain(f_gp), dl, _plain(u0), load=load, **opts)
    info = solver.solve()
    return solver.solution, info


class _SolveFn(torch.autograd.Function):
    """u* = solution of Z (K_nu u~ - F f) = 0, differentiable wrt nu and nodal f by the implicit-function theorem: for a cotangent g,
    lambda solves K_nu lambda = Z g with homogeneous conditions (the operator is symmetric), and
        dL/dnu = -d<lambda, R>/dnu,   dL/df = -d<lambda, R>/df    for R = Z (K_nu u~ - F f)
    which is one dn_poisson_coef_grad launch with v = lambda, a_nu = -1, a_f = +1 (include/diffnet_hip.h, the "residual R" line)."""

    @staticmethod
    def forward(ctx, nu, f, cfg):
        u, info = _solve_plain(cfg.geom, cfg.B, nu, f, cfg.f_gp, cfg.dl, cfg.u0, None, cfg.opts)
        info.adjoint = None
        cfg.info = info
        ctx.cfg = cfg
        ctx.shapes = (None if nu is None else nu.shape, None if f is None else f.shape)
        ctx.save_for_backward(u, _plain(nu))
        return u

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        cfg = ctx.cfg
        u, nu = ctx.saved_tensors
        homog = [Dirichlet(d.mask, 0.0) for d in cfg.dl]
        lam, info = _solve_plain(cfg.geom, cfg.B, nu, None, None, homog, None, g.to(torch.float32).contiguous(), cfg.opts)
        cfg.info.adjoint = info                # the adjoint solve's status, for whoever holds the forward info
        want = [k for k, need in zip(("nu", "f"), ctx.needs_input_grad[:2]) if need]
        g_nu, g_f = ops.poisson_coef_grad(cfg.geom, u, v=lam, dirichlet=cfg.dl, a_nu=-1.0, a_f=1.0, wscale=cfg.opts.get("jac", 1.0), want=want)
        outs = []
        for gr, shp in zip((g_nu, g_f), ctx.shapes):
            if gr is not None and shp[0] == 1 and gr.shape[0] != 1:
                gr = gr.sum(0, keepdim=True)           # a shared field receives the sum over the samples
            outs.append(gr)
        return outs[0], outs[1], None


def poisson_solve(geom, nu=None, f=None, f_gp=None, dirichlet=(), u0=None, batch=None, **options):
    """(u, info): the discrete solution of the Q1 Poisson problem for a batch, by preconditioned CG on the fused operator (Jacobi unless
    precondition="multigrid").

    Arguments as `PoissonSolver` (options: jac, tol, atol, maxiter, check_every, precondition, phases, mg_sweeps, mg_omega,
    mg_coarse_sweeps, mg_max_levels, mg_coarsening); batch: taken from the tensors when None.  info: `PoissonSolver.status()` of the last check plus `maxiter` -- look at info.converged: reaching maxiter does not raise.
    u is differentiable wrt `nu` and nodal `f` when they require a gradient (implicit differentiation: one more solve with the same
    options and a zero initial guess, then one dn_poisson_coef_grad launch; a shared (1,1,*N) field receives the sum over the
    samples).  There is NO gradient for f_gp, Dirichlet value fields or u0: a DiffNetHipError is raised if one of them requires one."""
    _check_geom(geom)
    dl = ops._norm_dirichlet(dirichlet)
    B = _infer_batch(geom, batch, nu, f, f_gp, u0, dl)
    grad_on = torch.is_grad_enabled()
    if grad_on and any(isinstance(t, torch.Tensor) and t.requires_grad for t in [f_gp, u0] + [d.value for d in dl]):
        raise DiffNetHipError("poisson_solve has no gradient for f_gp, Dirichlet value fields or u0 (only for nu and nodal f): detach them")
    pdl = _plain_conditions(dl)
    need = grad_on and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (nu, f))
    if need and isinstance(f, ops.LoadVector):
        raise DiffNetHipError("poisson_solve differentiates nodal forcing, not an assembled LoadVector")
    if not need:
        u, info = _solve_plain(geom, B, nu, f, f_gp, pdl, u0, None, options)
        return u, info
    if f_gp is not None and f is not None:
        raise ValueError("give either nodal f or f_gp, not both")
    cfg = types.SimpleNamespace(geom=geom, B=B, f_gp=f_gp, dl=pdl, u0=u0, opts=dict(options), info=None)
    u = _SolveFn.apply(nu, f, cfg)
    return u, cfg.info                # info.adjoint: the adjoint solve's status once the backward pass has run
