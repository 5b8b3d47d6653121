"""GPU tests of the host call path of the plate, flow, transport and element operators of diffnet_amd/ops.py (fsdt_apply, stokes_apply,
ns_apply, transport_apply, strongform_apply, fosls_apply, helmholtz_apply, eikonal_apply, eikonal3d_apply): the prepared-call cache directly -- a
miss, then a hit; a hit reads the buffers as they are now; a call that needs a conversion copy is not cached and agrees bitwise; the LRU
bound; call_cache_clear() -- and the type of every argument error, all of which are raised before a launch.

The meshes are the smallest that tell the axes apart: 9 x 7 nodes (Q1 with 2 Gauss points per axis; Q2 with 3 for the element operators),
6 x 5 x 4 nodes in 3-D, two samples.  Every call has a shared uint8 mask as condition 1, a per-sample fp32 mask with a per-sample value
field as condition 2, a Gauss-point forcing and its reductions on (fsdt_apply, with one mask and no forcing: condition 2 only); the
operators with a VJP mode are called in both modes."""
import pytest
import torch

from test_gpu_parity import cu, dev, module, seeded

pytestmark = pytest.mark.gpu

B = 2
LENGTHS = (1.0, 0.75, 0.5)


def _geom(nodes, deg, ngp):
    kw = dict(domain_sizes=nodes, domain_lengths=LENGTHS[:len(nodes)], domain_size=nodes[0], domain_length=LENGTHS[0], fem_basis_deg=deg, ngp_1d=ngp)
    if len(nodes) == 3:
        kw["nsd"] = 3
    return module(kw).geom


MESHES = {"q1": ((9, 7), 1, 2), "q2": ((9, 7), 2, 3), "3d": ((6, 5, 4), 1, 2)}


def _inputs(geom, vjp, nscale):
    """The arguments every case draws from; `u` is the buffer the tests change"""
    shape = (B, 1, *geom.node_shape)
    a = {k: cu(seeded(shape, s) - 0.5) for s, k in enumerate(("u", "v", "p", "mx", "my", "val2"))}
    m1 = torch.zeros((1, 1, *geom.node_shape), dtype=torch.uint8)
    m1[..., 0] = 1
    a["m1"] = m1.to(dev())
    a["m2"] = cu((seeded(shape, 11) < 0.2).float())
    a["fgp"] = cu(seeded((B, geom.ngp_total, *geom.elem_shape), 12))
    a["f"] = None
    a["cot"] = a["in_num"] = a["in_den"] = None
    if vjp:
        a["cot"] = tuple(cu(seeded(shape, 20 + k) - 0.5) for k in range(nscale))
        a["in_num"] = cu(1.0 + seeded((nscale,), 30))
        a["in_den"] = cu(2.0 + seeded((nscale,), 31))
    return a


def _stokes(ops, g, a):
    return ops.stokes_apply(g, a["u"], a["v"], a["p"], bc=(a["m1"], a["m2"], None), bc_values=(0.0, a["val2"], 0.0), visco=0.7, pspg=0.05,
                            f_gp=(a["fgp"], None), want_norms=True, in_num=a["in_num"], in_den=a["in_den"])


def _ns(ops, g, a):
    return ops.ns_apply(g, a["u"], a["v"], a["p"], bc=(a["m1"], a["m2"], None), bc_values=(0.0, a["val2"], 0.0), visco=0.7, f_gp=(a["fgp"], None),
                        cot=a["cot"], want_norms=True, in_num=a["in_num"], in_den=a["in_den"])


def _transport(ops, g, a):
    return ops.transport_apply(g, a["u"], bc=(a["m1"], a["m2"]), bc_values=(0.0, a["val2"]), f_gp=a["fgp"], adv=(0.8, 0.6), kappa=(0.1, 0.2),
                               tau=0.05, react=(0.1, 0.2, 0.3, 0.4), cot=a["cot"] and a["cot"][0], want_norm=True, in_num=a["in_num"],
                               in_den=a["in_den"])


def _strongform(ops, g, a):
    return ops.strongform_apply(g, a["u"], bc=(a["m1"], a["m2"]), bc_values=(0.0, a["val2"]), f=a["f"], f_gp=a["fgp"],
                                coef=(0.5, 0.25, 1.0, 0.1, 0.2, 1.0))


def _fosls(ops, g, a):
    return ops.fosls_apply(g, a["u"], a["mx"], a["my"], bc=(a["m1"], a["m2"]), bc_values=(0.0, a["val2"]), f=a["f"], f_gp=a["fgp"])


def _helmholtz(ops, g, a):
    return ops.helmholtz_apply(g, a["u"], sigma=0.5, bc=(a["m1"], a["m2"]), bc_values=(0.0, a["val2"]), f=a["f"], f_gp=a["fgp"], want_sumsq=True)


def _eikonal(ops, g, a):
    fn = ops.eikonal3d_apply if g.nsd == 3 else ops.eikonal_apply
    return fn(g, a["u"], bc=(a["m1"], a["m2"]), bc_values=(0.0, a["val2"]), f=a["f"], f_gp=a["fgp"], tau=0.25, cot=a["cot"] and a["cot"][0],
              in_num=a["in_num"], in_den=a["in_den"], want_sumsq=True, want_norm=True)


FSDT_CONSTS = dict(D11=1.0, D12=0.3, D22=1.2, D66=0.35, A44=0.8, A55=0.9, q=1.0, wscale=0.01)


def _fsdt(ops, g, a):
    """One mask (the per-sample one, `m2`), the value field on the second of the three fields; `in_num` / `in_den` where the case has them"""
    return ops.fsdt_apply(g, a["u"], a["v"], a["p"], a["m2"], (0.0, a["val2"], 0.0), want_sums=True, want_norms=True, in_num=a["in_num"],
                          in_den=a["in_den"], **FSDT_CONSTS)


# id: (operator object's name in ops, caller, mesh, VJP mode, length of in_num / in_den or None, takes nodal f)
CASES = {
    "fsdt_q1": ("_FSDT", _fsdt, "q1", False, 3, False),
    "fsdt_q2": ("_FSDT", _fsdt, "q2", False, 3, False),
    "fsdt_scaled_q2": ("_FSDT", _fsdt, "q2", True, 3, False),
    "fsdt_bool_mask_q2": ("_FSDT", _fsdt, "q2", False, 3, False),
    "stokes": ("_STOKES", _stokes, "q1", False, 3, False),
    "ns": ("_NS", _ns, "q1", False, 3, False),
    "ns_vjp": ("_NS", _ns, "q1", True, 3, False),
    "transport": ("_TRANSPORT", _transport, "q1", False, 1, False),
    "transport_vjp": ("_TRANSPORT", _transport, "q1", True, 1, False),
    "strongform_q1": ("_STRONGFORM", _strongform, "q1", False, None, True),
    "strongform_q2": ("_STRONGFORM", _strongform, "q2", False, None, True),
    "fosls_q1": ("_FOSLS", _fosls, "q1", False, None, True),
    "fosls_q2": ("_FOSLS", _fosls, "q2", False, None, True),
    "helmholtz_q1": ("_HELMHOLTZ", _helmholtz, "q1", False, None, True),
    "helmholtz_q2": ("_HELMHOLTZ", _helmholtz, "q2", False, None, True),
    "eikonal_q1": ("_EIKONAL", _eikonal, "q1", False, 1, True),
    "eikonal_q2": ("_EIKONAL", _eikonal, "q2", False, 1, True),
    "eikonal_vjp_q1": ("_EIKONAL", _eikonal, "q1", True, 1, True),
    "eikonal_vjp_q2": ("_EIKONAL", _eikonal, "q2", True, 1, True),
    "eikonal3d": ("_EIKONAL3D", _eikonal, "3d", False, 1, True),
    "eikonal3d_vjp": ("_EIKONAL3D", _eikonal, "3d", True, 1, True),
}
OPERATORS = ("_STOKES", "_NS", "_TRANSPORT", "_STRONGFORM", "_FOSLS", "_HELMHOLTZ", "_EIKONAL", "_EIKONAL3D", "_FSDT", "_POISSON", "_FDM_POISSON")


class Case:
    def __init__(self, name):
        from diffnet_amd import ops
        self.opname, self.fn, mesh, self.vjp, self.nscale, self.nodal_f = CASES[name]
        self.ops, self.op = ops, getattr(ops, self.opname)
        self.geom = _geom(*MESHES[mesh])
        self.args = _inputs(self.geom, self.vjp, self.nscale)
        if name == "fsdt_bool_mask_q2":
            self.args["m2"] = self.args["m2"] > 0.5

    def __call__(self, **over):
        """The results of one call as a flat list of tensors, with `over` replacing arguments"""
        out = []

        def flat(r):
            for x in r:
                if isinstance(x, (tuple, list)):
                    flat(x)
                elif x is not None:
                    out.append(x)

        flat(self.fn(self.ops, self.geom, {**self.args, **over}))
        return out

    def stats(self):
        s = dict(self.ops._CALL_STATS)
        for k in self.ops._CALL_STATS:
            self.ops._CALL_STATS[k] = 0
        return s

    def clear(self):
        self.ops.call_cache_clear()
        self.stats()


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", CASES)
def test_miss_then_hit(name):
    c = Case(name)
    c.clear()
    r1, r2 = c(), c()
    assert c.stats() == {"miss": 1, "hit": 1, "uncached": 0}
    assert len(c.op.cache) == 1
    assert len(r1) >= 2 and _same(r1, r2)
    assert all(torch.isfinite(x).all() for x in r1)
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(r1, r2))


@pytest.mark.parametrize("name", CASES)
def test_a_hit_follows_its_buffers(name):
    c = Case(name)
    c.clear()
    r1 = c()
    c.args["u"].mul_(0.5)
    c.stats()
    r2 = c()
    assert c.stats() == {"miss": 0, "hit": 1, "uncached": 0}
    c.clear()
    r3 = c()
    assert c.stats() == {"miss": 1, "hit": 0, "uncached": 0}
    assert _same(r2, r3)
    assert not torch.equal(r1[0], r2[0]) and not torch.equal(r1[-1], r2[-1])         # the field output and a reduction


@pytest.mark.parametrize("name", CASES)
def test_uncached_calls_agree(name):
    c = Case(name)
    c.clear()
    ref = c()
    u = c.args["u"]
    wide = torch.zeros((*u.shape[:-1], 2 * u.shape[-1]), dtype=u.dtype, device=u.device)
    view = wide[..., ::2]
    view.copy_(u)
    assert view.shape == u.shape and not view.is_contiguous()
    c.stats()
    got = c(u=view)
    assert c.stats() == {"miss": 0, "hit": 0, "uncached": 1}
    assert len(c.op.cache) == 1                # the contiguous call's entry only
    assert _same(got, ref)


@pytest.mark.parametrize("name", CASES)
def test_lru_bound_holds(name):
    c = Case(name)
    c.clear()
    n = c.ops._CALL_CACHE_MAX + 1
    us = [c.args["u"].clone() for _ in range(n)]            # all alive: n distinct buffers
    for u in us:
        c(u=u)
    assert c.stats() == {"miss": n, "hit": 0, "uncached": 0}
    assert len(c.op.cache) == c.ops._CALL_CACHE_MAX
    c(u=us[-1])
    c(u=us[0])                                               # the oldest entry was the one evicted
    assert c.stats() == {"miss": 1, "hit": 1, "uncached": 0}


def test_call_cache_clear_clears_every_operator():
    from diffnet_amd import ops
    objs = [getattr(ops, n) for n in OPERATORS]
    assert len({id(o) for o in objs}) == len(objs) and ops._EIKONAL3D.args_type is ops._EIKONAL.args_type
    for name in ("stokes", "ns", "transport", "strongform_q1", "fosls_q1", "helmholtz_q1", "eikonal_q1", "eikonal3d", "fsdt_q1"):
        Case(name)()
    c = Case("strongform_q1")
    ops.energy_loss_and_grad(c.geom, c.args["u"], dirichlet=[(c.args["m1"], 0.0)])
    ops.fdm_poisson_apply(c.args["u"])
    for n, o in zip(OPERATORS, objs):
        assert len(o.cache) >= 1 and len(o.ws_bytes) >= 1 and len(o.ws) >= 1, n
    ops.call_cache_clear()
    for n, o in zip(OPERATORS, objs):
        assert len(o.cache) == 0 and len(o.ws_bytes) == 0, n


def test_fsdt_bool_mask_equals_uint8_mask():
    c = Case("fsdt_bool_mask_q2")
    assert c.args["m2"].dtype == torch.bool
    c.clear()
    assert _same(c(), c(m2=c.args["m2"].to(torch.uint8)))
    assert c.stats() == {"miss": 2, "hit": 0, "uncached": 0}


def test_fsdt_deferred_pair_through_the_cache():
    """A defer_norms launch and the norms_from launch that consumes its partials, twice on the same buffers (a miss, then a hit, for each
    of the two calls): the same bits as the two-call form with in-kernel norms, with a Stokes launch between the two calls or without"""
    c, stokes = Case("fsdt_q2"), Case("stokes")
    ops, g, a = c.ops, c.geom, c.args
    flds, bc, vals = (a["u"], a["v"], a["p"]), a["m2"], (0.0, a["val2"], 0.0)
    wts = cu(torch.tensor([1.0, 2.0, 0.5]))
    vconsts = dict(FSDT_CONSTS, q=0.0)
    c.clear()
    R0, _, n0 = ops.fsdt_apply(g, *flds, bc, vals, want_sums=False, want_norms=True, **FSDT_CONSTS)
    g0, _ = ops.fsdt_apply(g, *R0, bc, (0.0, 0.0, 0.0), want_sums=False, in_num=wts, in_den=n0, **vconsts)
    ref = [*R0, *g0, n0]
    assert all(torch.isfinite(x).all() for x in ref) and float(n0.min()) > 0.0
    Rbuf = [torch.empty_like(x) for x in R0]                # the consumer's fields: the same buffers in both pairs
    c.clear()
    # (the Stokes launch of the second pair is a miss of its own)
    for between, want in ((False, {"miss": 2, "hit": 0, "uncached": 0}), (True, {"miss": 1, "hit": 2, "uncached": 0})):
        R, none, h = ops.fsdt_apply(g, *flds, bc, vals, want_sums=False, defer_norms=True, **FSDT_CONSTS)
        assert none is None and h.ws is c.op.ws[(torch.cuda.current_device(), ops._raw_stream(a["u"].device))]
        for dst, src in zip(Rbuf, R):
            dst.copy_(src)
        if between:
            assert all(torch.isfinite(x).all() for x in stokes())       # reduces in a workspace of its own
        G, _, n = ops.fsdt_apply(g, *Rbuf, bc, (0.0, 0.0, 0.0), want_sums=False, want_norms=True, in_num=wts, norms_from=h, **vconsts)
        assert c.stats() == want
        assert _same([*R, *G, n], ref), between


def _swapped(t):
    """`t` with its last two axes exchanged in the shape (and, in 3-D, its first two mesh axes): as many entries, the wrong mesh"""
    yield t.reshape(*t.shape[:-2], t.shape[-1], t.shape[-2])
    if t.dim() == 5:
        yield t.reshape(*t.shape[:-3], t.shape[-2], t.shape[-3], t.shape[-1])


@pytest.mark.parametrize("name", CASES)
def test_argument_errors_keep_their_type(name):
    from diffnet_amd._lib import DiffNetHipError
    c = Case(name)
    a = c.args
    c.clear()
    ref = c()
    fsdt = c.opname == "_FSDT"                               # one mask (m2), no forcing: the checks of m1, fgp and f do not apply
    if fsdt:
        assert len(c(m2=None)) == len(ref)                   # fsdt_apply reads bc_values only under a mask: no error, as ever
    else:
        with pytest.raises(ValueError):
            c(m2=None)                                       # a value field without its mask
        with pytest.raises(DiffNetHipError):
            c(m1=a["m1"].cpu())
        with pytest.raises(TypeError):
            c(m1=1.0)
    with pytest.raises(DiffNetHipError, match="fsdt_apply: bc mask must be on the GPU" if fsdt else None):
        c(m2=a["m2"].cpu())
    with pytest.raises(TypeError):
        c(m2=a["m2"].cpu().numpy())
    for key in ("m2", "val2") if fsdt else ("m1", "m2", "val2", "fgp"):
        for bad in _swapped(a[key]):
            assert bad.shape != a[key].shape
            with pytest.raises(ValueError):
                c(**{key: bad})
    if c.nodal_f:
        with pytest.raises(ValueError):
            c(f=a["val2"])                                   # nodal f together with a Gauss-point tensor
    if c.nscale is not None:
        ones = torch.ones(c.nscale, device=dev())
        with pytest.raises(ValueError):
            c(in_num=None, in_den=ones)
        with pytest.raises(ValueError):
            c(in_num=torch.ones(c.nscale + 1, device=dev()), in_den=ones)
    assert _same(c(), ref)                                   # none of them left anything behind in the cached call
