"""CPU checks of the winding-number VJP (dn_winding_field_vjp, csrc/winding_vjp.hip; ops.winding_field_vjp; diffnet_amd/winding.py): the
C ABI and its ctypes binding agree, the library validates its arguments before any launch, the workspace size and the automatic slice
count are what the header says, the composed torch route equals the float64 restatement (tests/winding_ref.py), passes gradcheck in
every argument and has torch's sgn(0) = 0 in its L1 gradient, and the `differentiable` keyword leaves the default untouched."""
import ctypes as C
import os

import pytest
import torch

import winding_ref as wr
import winding_vjp_ref as vr

SYMBOLS = ("dn_winding_field_vjp_slices", "dn_winding_field_vjp_workspace_bytes", "dn_winding_field_vjp")


def test_vjp_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "..", "include", "diffnet_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(h, s) and s in _lib.SYMBOLS and s + "(" in header, s
    assert "int64_t dn_winding_field_vjp_workspace_bytes(int32_t batch, int32_t npts, int32_t dim, int32_t slices);" in header
    assert "int dn_winding_field_vjp_slices(int32_t batch, int32_t npts, int64_t nq);" in header
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    assert "#define DN_ABI_VERSION 10" in header
    assert "winding_vjp.hip" in build.SOURCES
    assert _lib.SYMBOLS["dn_winding_field_vjp_workspace_bytes"][0] is C.c_int64
    assert len(_lib.SYMBOLS["dn_winding_field_vjp"][1]) == 19


def call(h, **kw):
    # every pointer is a small odd number: a check that came after a launch or a dereference would not return
    a = dict(points=17, normals=33, area=65, queries=129, grad_field=257, grad_points=513, grad_normals=1025, grad_area=2049,
             workspace=None, workspace_bytes=0, batch=2, npts=300, nq=1000, dim=3, metric=0, power=3, scale=1.0, slices=1, stream=None)
    a.update(kw)
    return h.dn_winding_field_vjp(a["points"], a["normals"], a["area"], a["queries"], a["grad_field"], a["grad_points"], a["grad_normals"],
                                  a["grad_area"], a["workspace"], a["workspace_bytes"], a["batch"], a["npts"], a["nq"], a["dim"], a["metric"],
                                  a["power"], a["scale"], a["slices"], a["stream"])


def test_vjp_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    for name in ("points", "normals", "queries", "grad_field"):                   # null required pointers
        assert call(h, **{name: None}) == -1, name
    assert call(h, grad_points=None, grad_normals=None, grad_area=None) == -1     # nothing to compute
    assert call(h, area=None) == -1                                               # grad_area without area
    for name, bad in (("dim", 1), ("dim", 4), ("metric", -1), ("metric", 2), ("power", 1), ("power", 4), ("batch", 0), ("batch", 65536),
                      ("npts", 0), ("npts", -5), ("nq", 0), ("nq", -1), ("slices", -1), ("slices", 1025)):
        assert call(h, **{name: bad}) == -1, (name, bad)
    # more than one effective slice needs a workspace: missing, or one byte short
    need = h.dn_winding_field_vjp_workspace_bytes(2, 300, 3, 4)
    assert need == 4 * 2 * 300 * 7 * 8
    assert call(h, slices=4) == -3
    assert call(h, slices=4, workspace=4097) == -3
    assert call(h, slices=4, workspace=4097, workspace_bytes=need - 1) == -3
    assert call(h, slices=0, nq=10 ** 6) == -3                                    # automatic: 1024 slices for this size
    assert h.dn_winding_field_vjp_slices(2, 300, 10 ** 6) == 1024 and h.dn_winding_field_vjp_slices(2, 300, 10 ** 5) == 391
    # the argument rules come before the workspace rule
    assert call(h, slices=4, points=None) == -1
    assert call(h, slices=4, workspace=4097, workspace_bytes=need, dim=5) == -1


def test_vjp_workspace_bytes():
    from diffnet_amd import _lib
    h = _lib.lib()
    for B, npts, dim, S in ((1, 1, 2, 1), (3, 257, 2, 5), (2, 300, 3, 4), (16, 1000, 2, 64), (1, 10242, 3, 1024), (65535, 1000, 3, 1024)):
        assert h.dn_winding_field_vjp_workspace_bytes(B, npts, dim, S) == S * B * npts * (1 + 2 * dim) * 8
    for bad in ((0, 10, 3, 1), (65536, 10, 3, 1), (1, 0, 3, 1), (1, 10, 1, 1), (1, 10, 4, 1), (1, 10, 3, 0), (1, 10, 3, 1025)):
        assert h.dn_winding_field_vjp_workspace_bytes(*bad) == -1, bad


def test_vjp_automatic_slices():
    from diffnet_amd import _lib
    f = _lib.lib().dn_winding_field_vjp_slices
    assert f(0, 10, 10) == f(1, 0, 10) == f(1, 10, 0) == -1
    # a cloud that fills the chip by itself (64 workgroups of 256 point threads on each of 256 CUs = 2^22) is not split
    assert f(1, 2 ** 22, 128 ** 3) == 1 and f(16, 2 ** 18, 128 ** 3) == 1 and f(1, 10 ** 7, 128 ** 3) == 1
    assert f(1, 2 ** 21, 128 ** 3) == 2 and f(1, 2 ** 18, 128 ** 3) == 16
    # never more than the chunks of 256 queries, never more than 1024
    for nq in (1, 255, 256, 257, 5000, 25 ** 3, 128 ** 3):
        chunks = (nq + 255) // 256
        for B, npts in ((1, 1), (1, 1000), (16, 1000), (1, 10242), (3, 70000), (1, 2 ** 22)):
            s = f(B, npts, nq)
            assert 1 <= s <= min(chunks, 1024), (B, npts, nq, s)
    assert f(1, 1, 128 ** 3) == 1024 and f(1, 1, 1000) == 4
    # monotone non-increasing in B Np
    for nq in (25 ** 3, 128 ** 3):
        sizes = sorted({B * npts: (B, npts) for B in (1, 2, 3, 16) for npts in (1, 100, 255, 256, 257, 1000, 10242, 100000, 3000000)}.items())
        got = [f(B, npts, nq) for _, (B, npts) in sizes]
        assert all(a >= b for a, b in zip(got, got[1:])), got
    assert f(1, 10242, 25 ** 3) == 62 and f(16, 1000, 64 ** 2) == 16 and f(1, 10242, 128 ** 3) == 410


@pytest.mark.parametrize("name", list(wr.PARAMS))
def test_composed_equals_the_restatement_in_float64(name):
    from diffnet_amd.winding import winding_field_composed
    p = wr.problem(name, 2, 37, 300)
    area = None if p["area"] is None else p["area"].double()
    for chunk in (4096, 128):
        w = winding_field_composed(p["points"].double(), p["normals"].double(), area, p["queries"].double(), p["metric"], p["power"],
                                   p["scale"], chunk=chunk)
        assert w.dtype == torch.float64 and tuple(w.shape) == (2, 300)
        assert float(((w - p["ref"]).abs() / p["A"]).max()) <= 1e-13
    # (B, Np, 1) areas and a query grid give the same values
    if area is not None:
        w2 = winding_field_composed(p["points"].double(), p["normals"].double(), area[..., None], p["queries"].double().reshape(-1, 20, 15),
                                    p["metric"], p["power"], p["scale"])
        assert float(((w2 - p["ref"]).abs() / p["A"]).max()) <= 1e-13


@pytest.mark.parametrize("name", list(wr.PARAMS))
def test_composed_gradcheck_in_every_argument(name):
    from diffnet_amd.winding import winding_field_composed
    p = wr.problem(name, 2, 7, 11)
    leaves = [p["points"].double().requires_grad_(True), p["normals"].double().requires_grad_(True), p["queries"].double().requires_grad_(True)]
    if p["area"] is not None:
        leaves.append(p["area"].double().requires_grad_(True))

    def f(pts, nrm, q, area=None):
        return winding_field_composed(pts, nrm, area, q, p["metric"], p["power"], p["scale"], chunk=4)

    assert torch.autograd.gradcheck(f, tuple(leaves))


@pytest.mark.parametrize("dim", [2, 3])
def test_composed_l1_gradient_is_zero_where_a_coordinate_coincides(dim):
    """point 0 and query 0 share coordinate 1 exactly: d|d_1|/dx_1 = sgn(0) = 0 (torch's convention), so that pair contributes only
    n_1 inv to the gradient of the point's coordinate 1"""
    from diffnet_amd.winding import winding_field_composed
    pts = torch.tensor([[0.30, 0.40, 0.55][:dim]], dtype=torch.float64)[None].requires_grad_(True)
    nrm = torch.tensor([[0.6, -0.8, 0.3][:dim]], dtype=torch.float64)[None]
    q = torch.tensor([[0.10, 0.40, 0.25][:dim]], dtype=torch.float64).T.contiguous()
    w = winding_field_composed(pts, nrm, None, q, "l1", 3, 1.0)
    (gp,) = torch.autograd.grad(w.sum(), pts)
    s = float((pts.detach()[0, 0] - q[:, 0]).abs().sum())
    assert float(gp[0, 0, 1]) == pytest.approx(float(nrm[0, 0, 1]) * s ** -3, rel=1e-14)
    # and the restatement the GPU tests use as their reference agrees
    (gr, _), _ = vr.vjp_reference(pts.detach(), nrm, None, q, torch.ones(1, 1, dtype=torch.float64), "l1", 3, 1.0)
    assert torch.allclose(gr, gp, rtol=1e-14, atol=0.0)


def test_vjp_reference_magnitudes_dominate_the_gradients():
    """the A of each output is a sum of absolute values of the terms whose sum the output is: it bounds the output"""
    for name in wr.PARAMS:
        v = vr.vjp_problem(name, 2, 37, 5)
        for out in ("points", "normals", "area"):
            if v["ref_" + out] is not None:
                assert bool((v["ref_" + out].abs() <= v["A_" + out] * (1 + 1e-12)).all()), (name, out)
                assert v["ref_" + out].shape == v["A_" + out].shape
        assert v["l1min"] >= wr.MIN_L1


def test_default_stays_detached_and_cpu_tensors_are_rejected():
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd import winding as W
    import inspect
    for fn in (W.winding_number, W.compute_winding_torch):
        assert inspect.signature(fn).parameters["differentiable"].default is False
    assert "differentiable" not in inspect.signature(W.winding_mask).parameters
    s = wr.sphere_problem(5, npts=50)
    pts, nrm, area = (s[k].clone().requires_grad_(True) for k in ("points", "normals", "area"))
    q5 = s["queries"][None]
    # the default path detaches what it hands to the kernel (the launch itself needs a GPU: test_gpu_winding_vjp.py)
    assert not any(t.requires_grad for t in W._cloud(pts, nrm, area))
    assert all(t.requires_grad for t in W._cloud(pts, nrm, area[..., None], detach=False))
    # differentiable=True on CPU tensors: the GPU-only error of the forward
    with pytest.raises(DiffNetHipError):
        W.winding_number(pts, nrm, area, s["queries"], differentiable=True)
    with pytest.raises(DiffNetHipError):
        W.compute_winding_torch(pts, nrm, area[..., None], q5, differentiable=True)
    with pytest.raises(DiffNetHipError):
        W.winding_field_ad(pts, nrm, area, s["queries"], "l2", 3, 1.0)
    # queries that require grad: a ValueError that names the composed route, before anything else
    qg = s["queries"].clone().requires_grad_(True)
    for fn, args in ((W.winding_number, (pts, nrm, area, qg)), (W.compute_winding_torch, (pts, nrm, area[..., None], qg[None]))):
        with pytest.raises(ValueError, match="winding_field_composed"):
            fn(*args, differentiable=True)
    with pytest.raises(ValueError, match="winding_field_composed"):
        W.winding_field_ad(pts, nrm, area, qg, "l2", 3, 1.0)


def test_ops_vjp_validates_before_the_device_check():
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.ops import winding_field_vjp
    p = wr.problem("3d_l1_p3_area", 2, 37, 5)
    g = torch.ones(2, 5)
    a = (p["points"], p["normals"], p["area"], p["queries"], g)
    with pytest.raises(DiffNetHipError):
        winding_field_vjp(*a)
    with pytest.raises(TypeError):
        winding_field_vjp(a[0].double(), *a[1:])
    with pytest.raises(ValueError):
        winding_field_vjp(*a[:4], torch.ones(2, 6))
    with pytest.raises(ValueError):
        winding_field_vjp(*a, want=())
    with pytest.raises(ValueError):
        winding_field_vjp(*a, want=("queries",))
    with pytest.raises(ValueError):
        winding_field_vjp(a[0], a[1], None, a[3], g, want=("area",))
    with pytest.raises(ValueError):
        winding_field_vjp(*a, slices=1025)
    with pytest.raises(ValueError):
        winding_field_vjp(*a, metric="linf")
    with pytest.raises(ValueError):
        winding_field_vjp(a[0], a[1].transpose(0, 1).contiguous().transpose(0, 1), *a[2:])
