"""The node a thread of the closed-form 2-D Q1 kernel shares with its right neighbour (poisson2d_q1_cf.hip: node x0 + 4 of u, nu and f),
on the launches where its route differs: one partly filled wave (8 nodes per row), the hand-over from lane 63 to lane 64 (260), three
waves in one chunk (516 on the default plan) and two chunks with a chunk-seam thread (516 under PLAN2D 128,4,R), rows of 4 k + 1 nodes
with the last node column in the last thread column (513); 19 and 35 node rows (strips with an odd tail; under the two-chunk plan the
strip height is chosen so that the last strip has one layer); B = 2; nu and f nodal, only nu, only f, neither; one condition as a
PackedMask and as a uint8 image.

The condition holds the boundary faces and single interior nodes at x = 3, 4, 255, 256, 257, 508, 511, 512 -- the nodes that are some
thread's shared node, or the first / last own node next to it -- and u differs there from the condition's value, so a neighbour's
element sees whether the value it was handed had the condition applied.

The public energy loss and its gradient
  - against the float64 oracle (loss rtol 1e-5, gradient rtol 1e-4 + 1e-4 max|ref|),
  - against the per-point kernel (Q1_RULE_KERNEL; it takes mask images, so it gets the uint8 image of the same nodes) at 2e-6:
the tolerances of test_gpu_q1cf_rowstaged.py."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import boundary_mask, dev, module, seeded
from test_gpu_switch_invariance import _kw2, _np, _oracle

pytestmark = pytest.mark.gpu

B = 2
C, JAC = 0.5, 0.7
VALUE, U_THERE = 0.25, -3.0
WIDTHS = {"8": 8, "260": 260, "516": 516, "516_two_chunks": 516, "513": 513}
HEIGHTS = (19, 35)
TERMS = {"nu_f": (True, True), "nu": (True, False), "f": (False, True), "none": (False, False)}
SPECIAL_X = (3, 4, 255, 256, 257, 508, 511, 512)


@pytest.fixture
def switch():
    from diffnet_amd import _lib
    held = []

    def set_(key, value):
        held.append(key)
        _lib.config_set(key, value)

    yield set_
    for key in held:
        _lib.config_set(key, "")


def _plan(width, ny):
    """two chunks of 128 threads, strips of R rows with (ny - 1) % R == 1: a one-layer last strip"""
    if width != "516_two_chunks":
        return None
    R = 17 if ny == 19 else 11
    assert (ny - 1) % R == 1
    return f"128,4,{R}"


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    kw = _kw2(nx, 3, sizes=(nx, ny))
    shape = (B, 1, *module(kw).geom.node_shape)
    assert shape[-1] == nx and shape[-2] == ny
    seed = 7000 + 3 * nx + ny
    u, nu, f = seeded(shape, seed), seeded(shape, seed + 1, 0.5), seeded(shape, seed + 2)
    mask = boundary_mask((1,) + shape[1:])
    for i, x in enumerate(SPECIAL_X):
        if not 0 < x < nx - 1:
            continue
        for y in ((3, 16, ny - 3) if i % 2 == 0 else (5, 17, ny - 4)):       # neighbouring columns on different rows: single nodes
            assert 0 < y < ny - 1
            mask[0, 0, y, x] = 1
    u = torch.where(mask.bool() & (boundary_mask((1,) + shape[1:]) == 0), torch.tensor(U_THERE), u)
    return kw, u, nu, f, mask


@functools.lru_cache(maxsize=None)
def _reference(nx, ny, has_nu, has_f):
    """float64 oracle: (loss, gradient)"""
    kw, u, nu, f, mask = _inputs(nx, ny)
    ur = u.double().requires_grad_(True)
    e = _oracle(kw).energy(ur, nu=nu.double() if has_nu else None, f=f.double() if has_f else None, dirichlet=[(mask.double(), VALUE)], c=C, jac=JAC)
    (g,) = torch.autograd.grad(e, ur)
    return float(e.detach()), _np(g)


def _public(m, u, nu, f, cond):
    ud = u.to(dev()).requires_grad_(True)
    loss = m.energy_loss(ud, None if nu is None else nu.to(dev()), None if f is None else f.to(dev()), dirichlet=[(cond, VALUE)], c=C, jac=JAC)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), _np(ud.grad)


@pytest.mark.parametrize("form", ["packed", "u8"])
@pytest.mark.parametrize("terms", sorted(TERMS))
@pytest.mark.parametrize("ny", HEIGHTS)
@pytest.mark.parametrize("width", sorted(WIDTHS))
def test_shared_node(width, ny, terms, form, switch):
    from diffnet_amd import PackedMask
    nx = WIDTHS[width]
    has_nu, has_f = TERMS[terms]
    kw, u, nu, f, mask = _inputs(nx, ny)
    m = module(kw)
    image = mask.to(dev()).to(torch.uint8)
    cond = PackedMask.pack(mask.to(dev())) if form == "packed" else image
    a = (u, nu if has_nu else None, f if has_f else None)
    tag = f"{nx} x {ny} ({width}) {terms} {form}"

    plan = _plan(width, ny)
    if plan:
        switch("PLAN2D", plan)
    loss, grad = _public(m, *a, cond)
    switch("PLAN2D", "")
    switch("Q1_RULE_KERNEL", "1")
    loss_pp, grad_pp = _public(m, *a, image)
    switch("Q1_RULE_KERNEL", "")
    loss_ref, grad_ref = _reference(nx, ny, has_nu, has_f)

    print(f"{tag}: loss {loss:.9g} per-point {loss_pp:.9g} oracle {loss_ref:.9g}; gradient: max|ref| {np.abs(grad_ref).max():.3g}, "
          f"max error against the per-point kernel {np.abs(grad - grad_pp).max():.3g}, against the oracle {np.abs(grad - grad_ref).max():.3g}")
    assert np.isfinite(grad).all(), f"{tag}: non-finite gradient (an output left unwritten)"
    on = np.broadcast_to(_np(mask) != 0, grad.shape)
    assert (grad[on] == 0).all(), f"{tag}: a gradient on a Dirichlet node"
    np.testing.assert_allclose(loss, loss_pp, rtol=2e-6, err_msg=f"{tag}: loss against the per-point kernel")
    np.testing.assert_allclose(grad, grad_pp, rtol=0, atol=2e-6 * max(1e-30, float(np.abs(grad_pp).max())), err_msg=f"{tag}: gradient against the per-point kernel")
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-5, err_msg=f"{tag}: loss against the float64 oracle")
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-4, atol=1e-4 * max(1e-30, float(np.abs(grad_ref).max())), err_msg=f"{tag}: gradient against the float64 oracle")
