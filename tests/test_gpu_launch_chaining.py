"""Launches that hand results to later launches -- a PoissonPlan fold, an FSDT defer_norms -> norms_from pair, the mask auto-pack cache -- and
the tuning switch that used to break them (include/diffnet_hip.h: chained results are "never silently stale").  Each test compares with the
float64 oracle or with the unchained launch, and names the quantity that would come out wrong."""
import numpy as np
import pytest
import torch

from test_gpu_parity import boundary_mask, close, dev, module, seeded

pytestmark = pytest.mark.gpu


def _blob(shape, seed, frac=0.05):
    return (seeded(shape, seed) < frac).float()


@pytest.fixture
def plan3d_e1():
    from diffnet_amd import _lib
    _lib.config_set("PLAN3D", "16,16,1,5")
    try:
        yield
    finally:
        _lib.config_set("PLAN3D", "")


def _oracle64(kw):
    from oracle.fem_oracle import Oracle
    o = Oracle(**kw)
    o.t = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in o.t.items()}
    o.gpw = o.gpw.double()
    return o


# ---------------------------------------------------------------------------------------------
# 1. PLAN3D with one element per thread on launches only the two-element form serves
# ---------------------------------------------------------------------------------------------
def test_plan3d_e1_keeps_box_faces_and_load_vector(plan3d_e1):
    """BoxFaces and a LoadVector under PLAN3D "16,16,1,5": equal to the oracle and, bitwise, to the same launch without the switch (the
    E = 1 override yields to the two-element form, which alone reads box faces and load vectors)."""
    from diffnet_amd import BoxFaces, LoadVector, _lib
    kw = dict(domain_size=34, nsd=3)
    m, o = module(kw), _oracle64(kw)
    shape = (2, 1, 34, 34, 34)
    u, nu, f = seeded(shape, 1), seeded(shape, 2, 0.5), seeded(shape, 3)
    box = boundary_mask(shape)
    obj = _blob((1, 1, 34, 34, 34), 4) * (1 - box[:1])
    ud, nud, fd = u.to(dev()), nu.to(dev()), f.to(dev())
    objd = obj.to(dev()).to(torch.uint8)
    lv = LoadVector.assemble(m.geom, fd)
    runs = {"box": ([(BoxFaces("all"), 0.0)], fd), "box+obj": ([(objd, 1.0), (BoxFaces("all"), 0.0)], fd),
            "load": ([(box.to(dev()).to(torch.uint8), 0.0)], lv)}
    refs = {"box": [(box.double(), 0.0)], "box+obj": [(obj.double(), 1.0), (box.double(), 0.0)], "load": [(box.double(), 0.0)]}
    got = {k: m.energy_loss_and_grad(ud, nud, ff, dirichlet=d, c=0.5, out=torch.full_like(ud, float("nan"))) for k, (d, ff) in runs.items()}
    _lib.config_set("PLAN3D", "")
    for k, (d, ff) in runs.items():
        ur = u.double().requires_grad_(True)
        ref = o.energy(ur, nu.double(), f.double(), dirichlet=refs[k], c=0.5)
        (gref,) = torch.autograd.grad(ref, ur)
        v, g = got[k]
        np.testing.assert_allclose(float(v), float(ref), rtol=1e-5, err_msg=f"{k}: loss under PLAN3D E=1 against the oracle")
        close(g, gref.numpy(), rtol=1e-4, arel=1e-4, msg=f"{k}: gradient under PLAN3D E=1 against the oracle")
        v0, g0 = m.energy_loss_and_grad(ud, nud, ff, dirichlet=d, c=0.5)
        assert torch.equal(v, v0), f"{k}: loss under PLAN3D E=1 {float(v)} != default {float(v0)}"
        assert torch.equal(g, g0), f"{k}: gradient under PLAN3D E=1 differs from the default launch"


@pytest.mark.parametrize("form", ["u8", "box"])
def test_plan3d_e1_fold_chain_writes_every_loss(plan3d_e1, form):
    """A pipelined chain of three with fold under PLAN3D "16,16,1,5": every evaluation's loss, sums and gradient equal the oracle; none is
    left at its -1 sentinel (the one-element form has no fold path)."""
    from diffnet_amd import BoxFaces, ops
    kw = dict(domain_size=34, nsd=3)
    m, o = module(kw), _oracle64(kw)
    B = 2
    shape = (B, 1, 34, 34, 34)
    box = boundary_mask((1, 1, 34, 34, 34))
    cond = (BoxFaces("all"), 0.0) if form == "box" else (box.to(dev()).to(torch.uint8), 0.0)
    scale = 1.0 / (B * m.geom.nelem_total)
    kwargs = dict(alpha=2.0, beta=1.0, c=1.0, wscale=1.0, out_scale=scale, want_out=True, want_sums=True, loss_scale=scale)
    sets = [(seeded(shape, 20 + 3 * k), seeded(shape, 21 + 3 * k, 0.5), seeded(shape, 22 + 3 * k)) for k in range(3)]
    plans = [ops.PoissonPlan(m.geom, *(t.to(dev()) for t in s), None, [cond], pipelined_sums=True, **kwargs) for s in sets]
    for k in (1, 2):
        plans[k].fold(plans[k - 1])
    for p in plans:
        p.result[0].fill_(float("nan"))
        p.result[1].fill_(-1.0)
        p.result[2].fill_(-1.0)
    for p in plans:
        p.launch()
    plans[2].finish_sums()
    torch.cuda.synchronize()
    for k, (u, nu, f) in enumerate(sets):
        ur = u.double().requires_grad_(True)
        ref = o.energy(ur, nu.double(), f.double(), dirichlet=[(box.double(), 0.0)], c=1.0)
        (gref,) = torch.autograd.grad(ref, ur)
        out, sums, loss = plans[k].result
        np.testing.assert_allclose(float(loss), float(ref), rtol=1e-5, err_msg=f"loss of evaluation {k} (-1: never written)")
        np.testing.assert_allclose(float(sums[0]) * scale, float(ref), rtol=1e-5, err_msg=f"energy of evaluation {k} (-1: never written)")
        close(out, gref.numpy(), rtol=1e-4, arel=1e-4, msg=f"gradient of evaluation {k}")


# ---------------------------------------------------------------------------------------------
# 2. FSDT defer_norms -> consumer with other reducing launches in between
# ---------------------------------------------------------------------------------------------
def _fsdt_setup():
    m = module(dict(domain_size=129, fem_basis_deg=2, ngp_1d=3))
    shape = (2, 1, 129, 129)
    flds = [seeded(shape, 100 + i).to(dev()) for i in range(3)]
    bcm = boundary_mask(shape).to(dev())
    consts = dict(D11=1.3, D12=0.4, D22=1.1, D66=0.6, A44=0.8, A55=0.9, q=1.2, wscale=0.3)
    wts = torch.tensor([1.0, 0.5, 2.0], device=dev())
    return m, flds, bcm, consts, wts


def test_poisson_launch_between_fsdt_defer_and_consumer_changes_nothing():
    """A reducing Poisson launch (one-shot energy_loss_and_grad on a large mesh: many partial sums) between an FSDT defer_norms launch and its
    norms_from consumer: the consumer's norms and gradients equal the uninterleaved pair bitwise."""
    from diffnet_amd import ops
    m, flds, bcm, consts, wts = _fsdt_setup()
    pm = module(dict(domain_size=513, ngp_1d=3))
    pshape = (2, 1, 513, 513)
    pu, pf = seeded(pshape, 120).to(dev()), seeded(pshape, 121).to(dev())
    pbc = boundary_mask(pshape).to(dev()).to(torch.uint8)

    def pair(interleave):
        Rs, _, h = ops.fsdt_apply(m.geom, *flds, bcm, want_sums=False, defer_norms=True, **consts)
        if interleave:
            ops.energy_loss_and_grad(pm.geom, pu, None, pf, None, [(pbc, 0.0)], c=1.0)
            ops.poisson_apply(pm.geom, pu, None, pf, None, [(pbc, 0.0)], alpha=1.0, beta=1.0, c=0.0, want_out=False, want_sums=True)
        c = dict(consts, q=0.0)
        g, _, n = ops.fsdt_apply(m.geom, *Rs, bcm, want_sums=False, want_norms=True, in_num=wts, norms_from=h, **c)
        return g, n

    g0, n0 = pair(False)
    g1, n1 = pair(True)
    assert torch.isfinite(n0).all()
    assert torch.equal(n0, n1), f"norms after an interleaved Poisson launch {n1.tolist()} != {n0.tolist()}"
    for k, (a, b) in enumerate(zip(g0, g1)):
        assert torch.equal(a, b), f"gradient {k} changed by an interleaved Poisson launch"


def test_fsdt_launch_between_fsdt_defer_and_consumer_gives_nan():
    """Another REDUCING FSDT launch in between clears the pair's ticket: the consumer's norms and outputs are NaN, never stale numbers."""
    from diffnet_amd import ops
    m, flds, bcm, consts, wts = _fsdt_setup()
    Rs, _, h = ops.fsdt_apply(m.geom, *flds, bcm, want_sums=False, defer_norms=True, **consts)
    ops.fsdt_apply(m.geom, *[t * 0.5 for t in flds], bcm, want_sums=True, **consts)
    g, _, n = ops.fsdt_apply(m.geom, *Rs, bcm, want_sums=False, want_norms=True, in_num=wts, norms_from=h, **dict(consts, q=0.0))
    assert torch.isnan(n).all(), f"norms after an interleaved reducing FSDT launch: {n.tolist()} (expected NaN)"
    assert all(torch.isnan(t).any() for t in g)


# ---------------------------------------------------------------------------------------------
# 3. fold across plans that do not match, and a fold by a launch without strips
# ---------------------------------------------------------------------------------------------
def _plans(kw, B, seed, **extra):
    from diffnet_amd import ops
    m = module(kw)
    shape = (B, 1, *m.geom.node_shape)
    scale = 1.0 / (B * m.geom.nelem_total)
    bc = boundary_mask((1,) + shape[1:]).to(torch.uint8).to(dev())
    u, nu, f = seeded(shape, seed).to(dev()), seeded(shape, seed + 1, 0.5).to(dev()), seeded(shape, seed + 2).to(dev())
    kwargs = dict(alpha=2.0, beta=1.0, c=1.0, wscale=1.0, out_scale=scale, want_out=True, want_sums=True, loss_scale=scale)
    kwargs.update(extra)
    return m, (u, nu, f, None, [(bc, 0.0)]), kwargs


def test_fold_refuses_a_plan_of_another_batch_mesh_or_stream():
    from diffnet_amd import ops
    from diffnet_amd._lib import DiffNetHipError
    m, a2, k2 = _plans(dict(domain_size=64, ngp_1d=3), 2, 30)
    _, a3, k3 = _plans(dict(domain_size=64, ngp_1d=3), 3, 40)
    m66, a66, k66 = _plans(dict(domain_size=66, ngp_1d=3), 2, 50)
    prev = ops.PoissonPlan(m.geom, *a2, pipelined_sums=True, **k2)
    with pytest.raises(DiffNetHipError, match="batch"):
        ops.PoissonPlan(m.geom, *a3, **k3).fold(prev)             # batch 3 folding batch 2: wrong partial count and stride
    with pytest.raises(DiffNetHipError, match="mesh"):
        ops.PoissonPlan(m66.geom, *a66, **k66).fold(prev)         # 66^2 folding 64^2
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.PoissonPlan(m.geom, *a2, **k2)
    with pytest.raises(DiffNetHipError, match="stream"):
        other.fold(prev)
    ops.PoissonPlan(m.geom, *a2, **k2).fold(prev)                  # same mesh, batch and stream: accepted


@pytest.mark.parametrize("kw", [dict(domain_sizes=(64, 3), domain_lengths=(1.0, 3 / 63), domain_size=64, ngp_1d=3),
                                dict(domain_sizes=(34, 10, 3), domain_lengths=(1.0, 9 / 33, 2 / 33), domain_size=34, nsd=3)],
                         ids=["2d_2rows", "3d_2layers"])
def test_fold_by_a_split_launch_without_strips_writes_prev_scalars(kw):
    """strip_select = 2 on a mesh of at most two strips launches no strip; a fold it carries must still form the folded evaluation's scalars."""
    from diffnet_amd import ops
    m, a, kwargs = _plans(kw, 1, 60)
    prev = ops.PoissonPlan(m.geom, *a, pipelined_sums=True, **kwargs)
    ref = [t.clone() for t in ops.PoissonPlan(m.geom, *a, **kwargs).launch()]
    nxt = ops.PoissonPlan(m.geom, *a, strip_select=2, **kwargs).fold(prev)
    prev.result[1].fill_(-1.0)
    prev.result[2].fill_(-1.0)
    prev.launch()
    nxt.launch()
    torch.cuda.synchronize()
    assert float(prev.result[2]) != -1.0, "loss of the folded evaluation was never written (sentinel -1)"
    np.testing.assert_allclose(float(prev.result[2]), float(ref[2]), rtol=1e-7, err_msg="loss of the folded evaluation")
    np.testing.assert_allclose(prev.result[1].cpu().numpy(), ref[1].cpu().numpy(), rtol=1e-13, err_msg="energy / sum of squares of the folded evaluation")


# ---------------------------------------------------------------------------------------------
# 4. mask auto-pack: inference tensors, streams
# ---------------------------------------------------------------------------------------------
def _autopack_setup():
    m = module(dict(domain_size=128, ngp_1d=3))
    shape = (2, 1, 128, 128)
    u, nu, f = seeded(shape, 301).to(dev()), seeded(shape, 302, 0.5).to(dev()), seeded(shape, 303).to(dev())
    box = boundary_mask(shape).to(dev())
    return m, u, nu, f, box


def _image_path(m, u, nu, f, cond):
    from diffnet_amd import ops
    ops.AUTO_PACK_MASKS = False
    try:
        return m.energy_loss_and_grad(u, nu, f, dirichlet=cond, c=1.0)
    finally:
        ops.AUTO_PACK_MASKS = True


def test_autopack_accepts_masks_made_under_inference_mode():
    from diffnet_amd import ops
    m, u, nu, f, box = _autopack_setup()
    ops.call_cache_clear()
    with torch.inference_mode():
        mask = box.clone()                                         # an inference tensor: no version counter
        v, g = m.energy_loss_and_grad(u, nu, f, dirichlet=[(mask, 0.0)], c=1.0)
        v2, g2 = m.energy_loss_and_grad(u, nu, f, dirichlet=[(mask, 0.0)], c=1.0)
    v0, g0 = _image_path(m, u, nu, f, [(box, 0.0)])
    np.testing.assert_allclose(float(v), float(v0), rtol=2e-6, err_msg="loss with an inference-mode mask")
    close(g, g0.cpu().numpy(), rtol=2e-6, arel=2e-6, msg="gradient with an inference-mode mask")
    assert torch.equal(v, v2) and torch.equal(g, g2)


def test_autopack_entry_is_per_stream():
    """The same mask used on a side stream after the default stream gets an entry of its own (packed on the side stream, so ordered
    before the launches there) and the same numbers."""
    from diffnet_amd import ops
    m, u, nu, f, box = _autopack_setup()
    ops.call_cache_clear()
    ops._PACK_STATS.update(hit=0, pack=0)
    v, g = m.energy_loss_and_grad(u, nu, f, dirichlet=[(box, 0.0)], c=1.0)
    assert ops._PACK_STATS == {"hit": 0, "pack": 1}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vs, gs = m.energy_loss_and_grad(u, nu, f, dirichlet=[(box, 0.0)], c=1.0)
        vs2, _ = m.energy_loss_and_grad(u, nu, f, dirichlet=[(box, 0.0)], c=1.0)
    torch.cuda.current_stream().wait_stream(side)
    assert ops._PACK_STATS == {"hit": 1, "pack": 2}, f"side-stream use of a mask packed on the default stream: {ops._PACK_STATS}"
    assert torch.equal(v, vs) and torch.equal(g, gs) and torch.equal(vs, vs2)
