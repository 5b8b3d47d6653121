"""Shared by test_winding_vjp_host.py and test_gpu_winding_vjp.py: the float64 reference of the winding-number VJP (autograd of
winding_ref.winding_general), the magnitude sums A of its three outputs, the rounding counts of the kernel's loop body (derivation:
header of test_gpu_winding_vjp.py) and the seeded cases.  No test lives here."""
import functools

import torch

import winding_ref as wr

CHUNK = 256               # csrc/winding_vjp.hip: queries staged per pass = length of one fp32 chain
# (B, npts, nq, slices): point counts around the workgroup's 256, query counts around the chunk, one and several slices, and more
# slices than chunks
SEAMS = [(1, 1, 255, 1), (2, 255, 1, 1), (3, 256, 257, 2), (2, 257, 3 * 256 + 5, 3), (3, 513, 1, 1), (1, 37, 5, 4)]


def n_roundings(dim, metric, power):
    """roundings on the longest path to one value of grad_normals / grad_area and of grad_points, in units of 2^-24"""
    if metric == "l1":
        e_r = dim + 2.0                                   # s: dim, v_rcp_f32: 2
        e_inv = power * e_r + (power - 1)
        e_x = e_r + 1                                     # r * (-power)
    else:
        e_rs = (2.0 + dim) / 2 + 2                        # r2: 2 + dim, v_rsq_f32 halves it and adds 2
        e_inv = power * e_rs + (power - 1)
        e_x = 2 * e_rs + 1 + 1                            # rs * rs, * (-power)
    e_gi = e_inv + 1                                      # g * inv
    n_normals = CHUNK + (1 + e_gi) + 2 + 1
    e_c = (1 + dim) + e_gi + 1 + e_x + 1 + (1 if metric == "l2" else 0)
    n_points = CHUNK + e_c + 2 + 1
    return n_normals, n_points


def vjp_reference(points, normals, area, queries, g, metric, power, scale, chunk=2048):
    """float64 (grad_points, grad_normals, grad_area | None) by autograd of winding_general with the cotangent g (B, nq), and the sums
    of absolute values (A_points, A_normals, A_area | None) of the terms of each output; all arguments float64"""
    leaves = [points.clone().requires_grad_(True), normals.clone().requires_grad_(True)]
    if area is not None:
        leaves.append(area.clone().requires_grad_(True))
    w, _ = wr.winding_general(leaves[0], leaves[1], leaves[2] if area is not None else None, queries, metric, power, scale)
    grads = torch.autograd.grad((w * g).sum(), leaves)
    a = torch.ones_like(points[..., 0]) if area is None else area
    Ap, An, Aa = torch.zeros_like(points), torch.zeros_like(points), torch.zeros_like(a)
    for q0 in range(0, queries.shape[1], chunk):
        q = queries[:, q0:q0 + chunk].T
        d = points[:, None, :, :] - q[None, :, None, :]                        # (B, nqc, Np, dim)
        ga = g[:, q0:q0 + chunk, None].abs()                                   # (B, nqc, 1)
        absnum = (d * normals[:, None]).abs().sum(-1)                          # sum_j |d_j n_j|
        if metric == "l1":
            s = d.abs().sum(-1)
            inv = s ** -power
            dinv = power * torch.sign(d).abs() * (s ** -(power + 1))[..., None]
        else:
            r = torch.sqrt((d * d).sum(-1))
            inv = r ** -power
            dinv = power * d.abs() * (r ** -(power + 2))[..., None]
        Aa += (ga * absnum * inv).sum(1)
        An += (ga[..., None] * d.abs() * inv[..., None]).sum(1)
        Ap += (ga[..., None] * (normals[:, None].abs() * inv[..., None] + absnum[..., None] * dinv)).sum(1)
    s = abs(scale)
    return grads, (s * a[..., None] * Ap, s * a[..., None] * An, s * Aa if area is not None else None)


@functools.lru_cache(maxsize=None)
def vjp_problem(name, B, npts, nq):
    """winding_ref.problem(name, B, npts, nq) with a seeded cotangent g = 2 rnd - 1 (float32), the float64 reference gradients, their
    A and the rounding counts; computed once and left unchanged"""
    p = wr.problem(name, B, npts, nq)
    dim, metric, power, _ = wr.PARAMS[name]
    g = (2.0 * wr.rnd((B, nq), "g", name, B, npts, nq) - 1.0).contiguous()
    area = None if p["area"] is None else p["area"].double()
    grads, As = vjp_reference(p["points"].double(), p["normals"].double(), area, p["queries"].double(), g.double(), metric, power, p["scale"])
    nn, np_ = n_roundings(dim, metric, power)
    return dict(p, g=g, ref_points=grads[0], ref_normals=grads[1], ref_area=grads[2] if area is not None else None,
                A_points=As[0], A_normals=As[1], A_area=As[2], n_points=np_, n_normals=nn, n_area=nn)
