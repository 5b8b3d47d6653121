"""Shared by test_winding_field_host.py and test_gpu_winding_field.py: the general winding-number formula restated in torch (float64
when given float64 inputs), its magnitude field, the rounding count of the kernel's loop body (derivation: header of
test_gpu_winding_field.py), the comparator and the seeded problems.  No test lives here."""
import functools
import math
import zlib

import torch

U = 2.0 ** -24            # unit roundoff of float32
CHUNK = 256               # csrc/winding_field.hip: points staged per pass
THREADS = 256             # threads per workgroup; a workgroup owns THREADS * tile queries
TILES = (1, 2, 4)
MIN_L1 = 1e-4
# (dim, metric, power, with area): the five parameter sets in use
PARAMS = {"2d_l1_p3": (2, "l1", 3, False), "2d_l1_p2_area": (2, "l1", 2, True), "3d_l1_p3_area": (3, "l1", 3, True),
          "2d_l2_p2": (2, "l2", 2, True), "3d_l2_p3": (3, "l2", 3, True)}


def winding_general(points, normals, area, queries, metric, power, scale, chunk=4096):
    """w[b, q] = scale sum_p area_p ((x_p - q) . n_p) / dist(x_p - q)^power and A[b, q], the same sum over the absolute values
    |scale| |area_p| sum_i |d_i n_i| / dist^power, in the dtype of the arguments.  points, normals (B, Np, dim); area (B, Np) or None;
    queries (dim, nq).  Returns two (B, nq) tensors."""
    ws, As = [], []
    a = torch.ones_like(points[..., 0]) if area is None else area
    for q0 in range(0, queries.shape[1], chunk):
        q = queries[:, q0:q0 + chunk].T                                        # (nqc, dim)
        d = points[:, None, :, :] - q[None, :, None, :]                        # (B, nqc, Np, dim)
        dist = d.abs().sum(-1) if metric == "l1" else torch.sqrt((d * d).sum(-1))
        dn = d * normals[:, None, :, :]
        ws.append(scale * (a[:, None, :] * dn.sum(-1) / dist ** power).sum(-1))
        As.append(abs(scale) * (a[:, None, :].abs() * dn.abs().sum(-1) / dist ** power).sum(-1))
    return torch.cat(ws, 1), torch.cat(As, 1)


def n_roundings(npts, dim, metric, power, has_area=True):
    """roundings on the longest path to one output of winding_field_kernel, in units of 2^-24 (see test_gpu_winding_field.py)"""
    if metric == "l1":
        den = power * dim + (power - 1) + 2
    else:
        den = power * ((2 + dim) / 2 + 2) + (power - 1)
    num = 1 + (1 if has_area else 0) + dim
    return npts + den + num + 2 + 1


def bound_ratio(got, ref, A, n):
    """max |got - ref| / (n 2^-24 A); inf where got is not finite or differs where A == 0"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    err, bound = (got - ref).abs(), n * U * A
    q = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    q = torch.where(torch.isfinite(got), q, torch.full_like(q, math.inf))
    return float(q.max())


def rnd(shape, *key):
    """seeded uniform values in (0, 1); the seed is a function of the key alone"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)
    return torch.rand(shape, generator=g)


def fibonacci_sphere(npts):
    """npts points on the unit sphere, a Fibonacci spiral (as examples/eikonal_3d.py), float64"""
    k = torch.arange(npts, dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * k / npts
    phi = math.pi * (1.0 + math.sqrt(5.0)) * k
    r = torch.sqrt(1.0 - z * z)
    return torch.stack((r * torch.cos(phi), r * torch.sin(phi), z), 1)


def cloud(B, npts, dim, *key):
    """float32 points on ellipses / ellipsoids whose centre and axes differ per sample, unit outward normals, areas that differ per
    point (mean = the curve's length or surface's area over npts, roughly)"""
    b = torch.arange(B, dtype=torch.float32)[:, None]
    ax = [0.27 + 0.031 * b, 0.21 - 0.017 * b, 0.24 + 0.011 * b][:dim]
    c = [0.4937 + 0.0113 * b, 0.4519 + 0.0071 * b, 0.5211 - 0.0057 * b][:dim]
    if dim == 2:
        th = torch.sort(rnd((B, npts), "th", B, npts, *key) * (2.0 * math.pi), dim=1).values
        unit = [torch.cos(th), torch.sin(th)]
    else:
        z = 2.0 * rnd((B, npts), "z", B, npts, *key) - 1.0
        ph = rnd((B, npts), "ph", B, npts, *key) * (2.0 * math.pi)
        r = torch.sqrt(1.0 - z * z)
        unit = [r * torch.cos(ph), r * torch.sin(ph), z]
    pts = torch.stack([c[i] + ax[i] * unit[i] for i in range(dim)], -1)
    nrm = torch.stack([unit[i] / ax[i] for i in range(dim)], -1)
    nrm = nrm / torch.linalg.vector_norm(nrm, dim=-1, keepdim=True)
    mean = (2.0 * math.pi * 0.24 if dim == 2 else 4.0 * math.pi * 0.24 ** 2) / npts
    area = mean * (0.5 + rnd((B, npts), "area", B, npts, *key))
    return pts.contiguous(), nrm.contiguous(), area.contiguous()


def default_scale(dim, metric, power):
    """the constants in use: (4 pi)^-3 for compute_winding_nodes' form, the solid-angle constants for the true winding number, else 1"""
    if metric == "l2":
        return 1.0 / (2.0 * (dim - 1) * math.pi)
    return (4.0 * math.pi) ** -3 if (dim, power) == (2, 3) else 1.0


def seam_cases(tile):
    """(B, npts, nq): every point count around the chunk, every query count around the workgroup's W = THREADS * tile, B = 1, 2, 3"""
    C, W = CHUNK, THREADS * tile
    return [(1, 1, W - 1), (2, C - 1, 1), (3, C, W + 1), (2, C + 1, 3 * W + 5), (3, 2 * C + 1, 1)]


@functools.lru_cache(maxsize=None)
def problem(name, B, npts, nq):
    """float32 inputs of a parameter set and, computed once and left unchanged, the float64 field, its magnitude field, the rounding
    count and the smallest L1 distance between a point and a query.  Queries are seeded points of the unit box."""
    dim, metric, power, has_area = PARAMS[name]
    pts, nrm, area = cloud(B, npts, dim, name, nq)
    if not has_area:
        area = None
    queries = rnd((dim, nq), "q", name, B, npts, nq).contiguous()
    for _ in range(3):                                   # a query that fell within 1e-3 (L1) of a point moves aside by 3.1e-3 in x
        near = (pts[:, None] - queries.T[None, :, None]).abs().sum(-1).amin((0, 2)) < 1e-3
        queries[0, near] += 3.1e-3
    scale = default_scale(dim, metric, power)
    ref, A = winding_general(pts.double(), nrm.double(), None if area is None else area.double(), queries.double(), metric, power, scale)
    l1 = (pts.double()[:, None] - queries.double().T[None, :, None]).abs().sum(-1).min()
    return dict(points=pts, normals=nrm, area=area, queries=queries, metric=metric, power=power, scale=scale, ref=ref, A=A,
                n=n_roundings(npts, dim, metric, power, has_area), l1min=float(l1))


@functools.lru_cache(maxsize=None)
def sphere_problem(n, npts=1000, radius=0.3):
    """the checked mask inputs: a Fibonacci sphere of npts points about the centre of the unit cube, equal areas 4 pi r^2 / npts, the
    n^3 nodes of the unit cube in mesh order; float64 true winding number (1, 1, n, n, n), A and the geometric inside"""
    unit = fibonacci_sphere(npts)
    pts = (0.5 + radius * unit).float()[None].contiguous()
    nrm = unit.float()[None].contiguous()
    area = torch.full((1, npts), 4.0 * math.pi * radius ** 2 / npts, dtype=torch.float32)
    x = torch.linspace(0.0, 1.0, n)
    zz, yy, xx = torch.meshgrid(x, x, x, indexing="ij")
    queries = torch.stack((xx, yy, zz)).contiguous()                           # (3, nz, ny, nx)
    w, A = winding_general(pts.double(), nrm.double(), area.double(), queries.reshape(3, -1).double(), "l2", 3, 1.0 / (4.0 * math.pi))
    inside = ((queries.double() - 0.5) ** 2).sum(0).sqrt() < radius
    return dict(points=pts, normals=nrm, area=area, queries=queries, w=w.reshape(1, 1, n, n, n), A=A.reshape(1, 1, n, n, n),
                inside=inside.reshape(1, 1, n, n, n), n=n_roundings(npts, 3, "l2", 3))
