#!/usr/bin/env python3
"""A fixed table of Poisson calls through ops.poisson_apply / ops.PoissonPlan: for each call the launch plan dn_poisson_query reports for
exactly the arguments that were launched (one line per call), and every result tensor saved to OUT.pt.  Run under
`rocprofv3 --kernel-trace` the trace gives (kernel name, grid, workgroup) per launch, to be held against the printed lines; run on two
trees the two OUT.pt files compare with torch.equal (tools/poisson_dispatch_trace.py --compare A.pt B.pt).  On a library without
dn_poisson_query the query lines are left out; the calls are the same.

    python tools/poisson_dispatch_trace.py OUT.pt
"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a, b):
    A, B = torch.load(a), torch.load(b)
    assert list(A) == list(B), "the two runs made different calls"
    bad = [k for k in A if not all(torch.equal(x, y) for x, y in zip(A[k], B[k])) or len(A[k]) != len(B[k])]
    n = sum(len(v) for v in A.values())
    finite = all(bool(torch.isfinite(t.double()).all()) for v in A.values() for t in v)
    print(f"{len(A)} calls, {n} tensors, all finite: {finite}, torch.equal on all but {len(bad)}", *bad, sep="\n")
    return 1 if bad or not finite else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

from diffnet_amd import BoxFaces, LoadVector, PackedMask, _lib, ops       # noqa: E402
from diffnet_amd.fem import FemGeometry                                    # noqa: E402
from diffnet_amd.tables import gauss_rule                                  # noqa: E402

dev = torch.device("cuda:0")
HAVE_QUERY = hasattr(_lib, "DnPoissonKernel")
saved = {}


def seeded(shape, seed, lo=0.0):
    return (lo + torch.rand(shape, generator=torch.Generator().manual_seed(seed))).to(dev)


def geometry(sizes, deg=1, ngp=2):
    gx, gw = gauss_rule(ngp)
    return FemGeometry(len(sizes), sizes, tuple(1.0 / (n - 1) for n in sizes), deg, ngp, gx, gw)


def report(name, mesh, args):
    if not HAVE_QUERY:
        return
    k = _lib.DnPoissonKernel()
    rc = _lib.lib().dn_poisson_query(C.byref(mesh), C.byref(args), C.byref(k))
    threads = k.tile[0] * max(k.tile[1], 1) * (k.W if k.W > 1 else 1)
    print(f"QUERY {name}: rc {rc} {_lib.POISSON_FAMILIES.get(k.family)} grid {k.launched} x {threads} threads  tile {k.tile[0]},{k.tile[1]} E {k.E} R {k.R} W {k.W} "
          f"ua {k.ua} vec {k.vec} chunks {k.chunks} tiles {k.tiles} strips {k.launched_strips}/{k.strips} stride {k.stride} ws {k.workspace_bytes} "
          f"compact {k.compact}")


def inputs(geom, B, mask, forcing, seed):
    """mask: none | u8 | f32 | field | packed | box | box+u8 | box+f32;  forcing: none | nodal | gp | load"""
    shape = (B, 1, *geom.node_shape)
    u, nu = seeded(shape, seed), seeded(shape, seed + 1, 0.5)
    f = seeded(shape, seed + 2) if forcing in ("nodal", "load") else None
    if forcing == "load":
        f = LoadVector.assemble(geom, f)
    f_gp = seeded((B, geom.ngp_total, *geom.elem_shape), seed + 3) if forcing == "gp" else None
    edge = torch.zeros((1,) + shape[1:])
    for d in range(geom.nsd):
        idx = [slice(None)] * len(shape)
        for side in (0, -1):
            idx[2 + d] = side
            edge[tuple(idx)] = 1
    edge = edge.to(dev)
    blob = ((seeded(shape, seed + 4) < 0.05) & (edge.expand(shape) == 0)).float()
    dl = {"none": [], "u8": [(blob.to(torch.uint8), 1.0), (edge.to(torch.uint8), 0.0)], "f32": [(edge, 0.0)],
          "field": [(edge, seeded((1,) + shape[1:], seed + 5))], "packed": [(PackedMask.pack(blob), 1.0), (PackedMask.pack(edge), 0.0)],
          "box": [(BoxFaces("all"), 0.0)], "box+u8": [(blob.to(torch.uint8), 1.0), (BoxFaces("all"), 0.0)],
          "box+f32": [(BoxFaces("all"), 0.0), (blob, 0.5)]}[mask]
    return u, nu, f, f_gp, dl


def keep(name, tensors):
    assert name not in saved, name
    saved[name] = [t.detach().clone().cpu() for t in tensors if isinstance(t, torch.Tensor)]


def one_shot(sizes, deg, ngp, B, mask, forcing, seed):
    """ops.poisson_apply (the call cache's miss path: packs mask images where the compact kernels take the call)"""
    geom = geometry(sizes, deg, ngp)
    name = f"apply {'x'.join(map(str, sizes))} Q{deg} ngp {ngp} B {B} mask {mask} f {forcing}"
    u, nu, f, f_gp, dl = inputs(geom, B, mask, forcing, seed)
    scale = 1.0 / (B * geom.nelem_total)
    ops.call_cache_clear()
    res = ops.poisson_apply(geom, u, nu, f, f_gp, dl, alpha=2.0, beta=1.0, c=1.0, out_scale=scale, loss_scale=scale)
    plan = next(reversed(ops._POISSON.cache.values()), None)              # the prepared call that was just launched
    if plan is not None:
        report(name, plan.mesh, plan.args)
    keep(name, res)


def planned(tag, sizes, ngp, B, mask, forcing, seed, **kw):
    geom = geometry(sizes, 1, ngp)
    name = f"plan {tag} {'x'.join(map(str, sizes))} ngp {ngp} B {B} mask {mask} f {forcing}"
    u, nu, f, f_gp, dl = inputs(geom, B, mask, forcing, seed)
    scale = 1.0 / (B * geom.nelem_total)
    plan = ops.PoissonPlan(geom, u, nu, f, f_gp, dl, alpha=2.0, beta=1.0, c=1.0, out_scale=scale, loss_scale=scale, **kw)
    return name, plan


Q1_2D = ["none/none", "u8/nodal", "f32/nodal", "field/none", "packed/nodal", "box/none", "box+u8/nodal", "u8/gp", "none/gp"]
Q1_3D = ["none/none", "u8/nodal", "f32/nodal", "field/nodal", "packed/none", "box/nodal", "box+u8/nodal", "box+f32/none", "u8/gp"]
LOADS = ["box/load", "u8/load", "none/load"]                               # the two-element 3-D kernels only: even nx, 2-point rule


def main(out_path):
    seed = 1000
    n = 0
    for sizes, ngp in (((64, 64), 2), ((65, 65), 3), ((66, 66), 2), ((72, 45), 4), ((130, 37), 2), ((97, 97), 3)):
        for i, combo in enumerate(Q1_2D):
            mask, forcing = combo.split("/")
            seed += 10
            one_shot(sizes, 1, ngp, 1 if (i + n) % 2 == 0 else 3, mask, forcing, seed)
        n += 1
    for i, combo in enumerate(["none/nodal", "u8/gp", "f32/none", "packed/nodal", "box/none"]):
        mask, forcing = combo.split("/")
        seed += 10
        one_shot((65, 65), 2, 3, 1 + 2 * (i % 2), mask, forcing, seed)
    for sizes, ngp in (((34, 34, 34), 2), ((34, 21, 11), 2), ((33, 33, 33), 2), ((17, 17, 17), 3), ((5, 4, 3), 2), ((6, 5, 3), 2)):
        for i, combo in enumerate(Q1_3D + (LOADS if sizes[0] % 2 == 0 and ngp == 2 else [])):
            mask, forcing = combo.split("/")
            seed += 10
            one_shot(sizes, 1, ngp, 1 if (i + n) % 2 == 0 else 3, mask, forcing, seed)
        n += 1
    for i, combo in enumerate(["none/nodal", "u8/gp", "f32/none"]):
        mask, forcing = combo.split("/")
        seed += 10
        one_shot((9, 7, 5), 2, 3, 1 + 2 * (i % 2), mask, forcing, seed)

    # prepared launches: chained strips (the plan picks them for 512-wide launches that do not fill the chip), split evaluation on a mesh with
    # many strips and on meshes with one or two, pipelined sums with a fold and the closing finish_sums
    name, plan = planned("chained", (512, 40), 3, 3, "packed", "nodal", 5000)
    report(name, plan.mesh, plan.args)
    keep(name, plan.launch())
    for sizes, ngp, mask in (((130, 37), 2, "u8"), ((64, 5), 2, "box"), ((34, 34, 34), 2, "box+u8"), ((6, 5, 3), 2, "u8"), ((33, 33, 33), 2, "f32")):
        seed += 10
        name, first = planned("split 1", sizes, ngp, 3, mask, "nodal", seed, strip_select=1)
        name2, second = planned("split 2", sizes, ngp, 3, mask, "nodal", seed, strip_select=2, continues=first)
        report(name, first.mesh, first.args)
        report(name2, second.mesh, second.args)
        first.launch()
        keep(name, second.launch())
    for sizes, ngp, mask in (((66, 66), 2, "u8"), ((512, 40), 2, "box"), ((34, 21, 11), 2, "box"), ((64, 5), 2, "packed")):
        plans = []
        for k in range(3):
            seed += 10
            plans.append(planned(f"pipelined {k}", sizes, ngp, 3, mask, "nodal", seed, pipelined_sums=True))
        for k in (1, 2):
            plans[k][1].fold(plans[k - 1][1])
        for name, plan in plans:
            report(name, plan.mesh, plan.args)
            plan.launch()
        plans[2][1].finish_sums()
        torch.cuda.synchronize()
        for name, plan in plans:
            keep(name, plan.result)
    torch.cuda.synchronize()
    torch.save(saved, out_path)
    print(f"{len(saved)} calls, {sum(len(v) for v in saved.values())} tensors saved to {out_path}; call cache {ops._CALL_STATS}")


if __name__ == "__main__":
    main(sys.argv[1])
