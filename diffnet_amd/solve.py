"""Batched matrix-free conjugate-gradient solve of the discrete Q1 Poisson problem  Z (K_nu u~ - F f) = 0  -- the field the energy and
residual losses of this library converge to -- and its implicit derivative with respect to the nodal coefficient and forcing.

One iteration is the fused operator (q = Z K_nu p through a prepared `ops.PoissonPlan`) followed by the three vector phases of
`dn_poisson_cg` (include/diffnet_hip.h): per-sample dot products become per-sample alpha / beta on the device, converged samples of a
batch stand still, and nothing of an iteration touches the host but the launches themselves: a chunk of iterations can be captured
with torch.cuda.graph.

Limits, stated plainly: Q1 meshes only (degree 1, rules of 2 to 4 points), Jacobi preconditioning only (or none).  Float32 CG stalls at
a relative residual that grows with the condition number of the mesh (README.md quotes measured levels); ask for a `tol` it can reach.
"""
import types

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import DiffNetHipError
from .ops import Dirichlet, PackedMask


def _check_geom(geom):
    if geom.deg != 1:
        raise DiffNetHipError(f"PoissonSolver: Q1 meshes only (fem_basis_deg = 1), got degree {geom.deg}: the CG kernels and the "
                              "Jacobi diagonal are written for the Q1 operator")
    if not 2 <= geom.ngp_1d <= 4:
        raise DiffNetHipError(f"PoissonSolver: rules of 2 to 4 points per axis, got {geom.ngp_1d}")


def _tensors_of(nu, f, f_gp, u0, dl, load=None):
    ts = [nu, f.tensor if isinstance(f, ops.LoadVector) else f, f_gp, u0, load]
    for d in dl:
        ts += [d.mask if isinstance(d.mask, torch.Tensor) else getattr(d.mask, "bits", None), d.value]
    return [t for t in ts if isinstance(t, torch.Tensor)]


class PoissonSolver:
    """Preconditioned CG on FIXED buffers for `batch` samples of one mesh.

        solver = PoissonSolver(geom, batch, nu=None, f=None, f_gp=None, dirichlet=(), u0=None, jac=1.0, tol=1e-5, atol=0.0,
                               maxiter=None, check_every=32, precondition="jacobi")
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
    n-node-wide mesh); `poisson_solve` stops there.  precondition: "jacobi" or None (dinv = 1 on the free nodes).
    load: an ASSEMBLED right-hand side (B,1,*N) added to F f (read as zero on the Dirichlet nodes): what the adjoint solve needs.
    phases: "fused" (the dn_poisson_cg kernels) or "composed" (the same recurrences from torch ops on `ops.residual`: a measuring
    stick, about a dozen launches per iteration)."""

    def __init__(self, geom, batch, nu=None, f=None, f_gp=None, dirichlet=(), u0=None, jac=1.0, tol=1e-5, atol=0.0, maxiter=None,
                 check_every=32, precondition="jacobi", load=None, phases="fused", device=None):
        _check_geom(geom)
        if precondition not in ("jacobi", None):
            raise ValueError('precondition must be "jacobi" or None')
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
        self.check_every = max(1, int(check_every))
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
        if phases == "fused":
            self.state = ops.poisson_cg_state(self.B, self.device)
            self.workspace = ops.poisson_cg_workspace(self.n, self.B, self.device)
            mk = lambda ph: ops.poisson_cg_args(ph, self.x, self.r, self.p, self.q, self.dinv, self.state, self.workspace, self.tol, self.atol)
            self._args = {ph: mk(ph) for ph in ("init", "dot", "update", "direction")}
            fn = _lib.lib().dn_poisson_cg
            refs = [ops.C.byref(self._args[ph][0]) for ph in ("dot", "update", "direction")]
            self._fn, self._refs = fn, refs
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
            self._plan0.launch()
            if self.load is not None:
                fx = self._fixed()
                ld = self.load.to(self.device).expand_as(self.q)
                self.q.sub_(ld if fx is None else torch.where(fx, torch.zeros_like(ld), ld))
            if self.phases == "fused":
                ops.poisson_cg_launch(self._args["init"][0], self.device)
            else:
                self._composed_init()
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
        for _ in range(int(k)):
            plan.launch()
            for ref in refs:
                rc = fn(ref, s)
                if rc:
                    _lib.check(rc, "dn_poisson_cg")
        return self

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

    def _composed_init(self):
        r = -self.q
        self.r.copy_(r)
        self.p.copy_(self.dinv * r)
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
        z = self.dinv * r
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
    """(u, info): the discrete solution of the Q1 Poisson problem for a batch, by Jacobi-preconditioned CG on the fused operator.

    Arguments as `PoissonSolver` (options: jac, tol, atol, maxiter, check_every, precondition, phases); batch: taken from the tensors when
    None.  info: `PoissonSolver.status()` of the last check plus `maxiter` -- look at info.converged: reaching maxiter does not raise.
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
