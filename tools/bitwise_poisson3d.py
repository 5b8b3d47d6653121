#!/usr/bin/env python3
"""SHA-256 of every output and scalar of one seeded case set of the fused Poisson operator on 3-D Q1 meshes, and of a handful of eikonal3d_apply
and gauss_pt_eval launches (the kernels that share dn_common.h's xcd_remap): one line per output, "<case> <output> <digest>".  Run it once per
library (DN_LIB_PATH selects one, one process each) and compare the two listings: `python tools/bitwise_poisson3d.py --compare A.txt B.txt`
prints the differing lines and the counts and exits 1 if any differ.

Cases: the argument sets of tests/test_gpu_poisson3d_forms.py (tests/poisson3d_ref.py: part 1, every instantiation the dispatch can pick in the
five families under "Q1_3D_E1", "Q1_3D_T16", "Q1_3D_N2", "Q1_3D_E1SUM" and "PLAN3D"; part 2, the seam meshes), each launched as that file
launches it after dn_poisson_query named the family the case is meant for; a launch without sums of the same arguments where the case wants
them; and per two-element family a pair of chained launches whose second one folds the first one's sums (dn_poisson_args.fold_prev).

Usage: python tools/bitwise_poisson3d.py OUT.txt
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
KEYS = ("Q1_3D_E1", "Q1_3D_T16", "Q1_3D_N2", "Q1_3D_E1SUM", "PLAN3D")


def digest(t):
    a = t if isinstance(t, np.ndarray) else t.detach().contiguous().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class Out:
    def __init__(self, path):
        self.fh = open(path, "w")
        self.cases = self.outputs = 0

    def case(self, name, **outs):
        self.cases += 1
        for k, t in outs.items():
            if t is not None:
                self.fh.write(f"{name} {k} {digest(t)}\n")
                self.outputs += 1
        self.fh.flush()


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def plan_of(p, c, want_sums, pipelined=False):
    """the PoissonPlan of a case (the construction of tests/test_gpu_poisson3d_forms.py: prepare), `out` filled with NaN"""
    import torch
    from diffnet_amd import ops
    from diffnet_amd.fem import FemGeometry
    gx, gw = p.rule_points(c["rule"])
    geom = FemGeometry(3, c["mesh"], p.HS, 1, c["ngp"], gx, gw)
    n5 = lambda a: _cu(a).unsqueeze(1)                  # noqa: E731
    dl = []
    for m in c["conds"]:
        v = n5(m["value"]) if isinstance(m["value"], np.ndarray) else m["value"]
        dl.append((ops.BoxFaces([n for n, b in p.FACES.items() if m["faces"] & b]) if m["kind"] == "box" else n5(m["img"]), v))
    f = fgp = None
    if c["fkind"] == "gp":
        fgp = _cu(c["f"])
    elif c["fkind"] == "nodal":
        f = n5(c["f"])
    elif c["fkind"] == "load":
        f = ops.LoadVector(n5(c["f"]))
    u = n5(c["u"])
    return ops.PoissonPlan(geom, u, None if c["nu"] is None else n5(c["nu"]), f, fgp, dl, c["alpha"], c["beta"], c["c"], c["wscale"], c["out_scale"],
                           want_out=True, want_sums=want_sums, loss_scale=c["energy_scale"] if want_sums else None, out=torch.full_like(u, float("nan")),
                           strict=True, pipelined_sums=pipelined)


def results(pl):
    import torch
    torch.cuda.synchronize()
    if pl.result[1] is None:
        return dict(out=pl.result[0])
    return dict(out=pl.result[0], sums=pl.result[1], energy_f32=pl.result[2])


def poisson_cases(out):
    import poisson3d_ref as p
    from diffnet_amd import _lib, ops
    folded = set()
    for case in p.all_cases():
        c = p.build(case)
        fam, _ = p.choose(c)
        for k in KEYS:
            _lib.config_set(k, dict(c["switches"], PLAN3D=c["plan"]).get(k, ""))
        ops.call_cache_clear()
        name = "poisson3d " + " ".join(str(x).replace(" ", "") for x in case)
        for ws in ((True, False) if c["want_sums"] else (False,)):
            pl = plan_of(p, c, ws)
            k = _lib.DnPoissonKernel()
            rc = _lib.lib().dn_poisson_query(C.byref(pl.mesh), C.byref(pl.args), C.byref(k))
            if rc != 0 or p.FAM.get(k.family) != fam:
                raise SystemExit(f"{name}: dn_poisson_query gives {rc}, family {p.FAM.get(k.family)}; the case is meant for {fam}")
            pl.launch()
            out.case(f"{name} sums={int(ws)} [{fam}]", **results(pl))
        # dn_poisson_args.fold_prev exists in the two-element kernels: once per family and kind of condition
        if fam in ("cfz", "n2") and c["want_sums"] and (fam, case.cond) not in folded:
            folded.add((fam, case.cond))
            a, b = plan_of(p, c, True, pipelined=True), plan_of(p, c, True, pipelined=True)
            a.launch()
            b.fold(a).launch()
            b.finish_sums()
            ra, rb = results(a), results(b)
            out.case(f"{name} fold_prev [{fam}]", out=rb["out"], folded_sums=ra["sums"], folded_energy_f32=ra["energy_f32"], sums=rb["sums"])
    for k in KEYS:
        _lib.config_set(k, "")
    ops.call_cache_clear()
    print(f"poisson3d: {out.cases} cases, {out.outputs} outputs so far", flush=True)


def rand(shape, seed, lo=-0.5):
    import torch
    return (lo + torch.rand(shape, generator=torch.Generator().manual_seed(seed))).to(DEV)


def neighbour_cases(out):
    """kernels whose 1-D grid decode became xcd_remap: meshes of more than 8 workgroups, a multiple of 8 and not"""
    import torch
    import poisson3d_ref as p
    from diffnet_amd import ops
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    for n, (mesh, B, ngp) in enumerate([((33, 33, 9), 1, 2), ((40, 37, 21), 3, 2), ((33, 18, 9), 2, 3), ((31, 31, 6), 3, 4)]):
        geom = FemGeometry(3, mesh, p.HS, 1, ngp, *gauss_rule(ngp))
        shape = (B, 1, mesh[2], mesh[1], mesh[0])
        u, cot = rand(shape, 100 + n), rand(shape, 200 + n)
        bc = ((rand(shape, 300 + n, 0.0) < 0.15).float(), (rand((1, *shape[1:]), 400 + n, 0.0) < 0.15).to(torch.uint8))
        name = f"eikonal3d {mesh} B={B} ngp={ngp}"
        R, s, nrm = ops.eikonal3d_apply(geom, u, bc, (0.3, -0.2), tau=0.05, wscale=0.37, want_sumsq=True, want_norm=True)
        out.case(name + " fwd", R=R, sumsq=s, norm=nrm)
        g, s, nrm = ops.eikonal3d_apply(geom, u, bc, (0.3, -0.2), tau=0.05, wscale=0.37, cot=cot, want_sumsq=True, want_norm=True)
        out.case(name + " vjp", g=g, sumsq=s, norm=nrm)
    for n, (nsd, mesh, B, G) in enumerate([(2, (130, 70), 3, 4), (2, (257, 129), 1, 9), (3, (40, 37, 21), 2, 8), (3, (33, 33, 9), 3, 27), (3, (66, 18, 5), 1, 8),
                                           (3, (9, 9, 9), 5, 8)]):
        u = rand((B, 1, *reversed(mesh)), 500 + n).requires_grad_(True)
        val = ops.gauss_pt_eval(u, rand((G, 2 ** nsd), 600 + n), nsd)
        (gu,) = torch.autograd.grad(val, u, rand(tuple(val.shape), 700 + n))
        out.case(f"gauss_pt_eval {nsd}-D {mesh} B={B} G={G}", val=val, grad_u=gu)
    print(f"with the neighbours: {out.cases} cases, {out.outputs} outputs", flush=True)


def compare(a, b):
    def load(p):
        d = {}
        for line in open(p):
            key, dig = line.rstrip("\n").rsplit(" ", 1)
            d[key] = dig
        return d
    A, B = load(a), load(b)
    if A.keys() != B.keys():
        print(f"the listings hold different outputs: {len(A.keys() ^ B.keys())} keys in one only")
        return 1
    bad = [k for k in A if A[k] != B[k]]
    for k in bad:
        print("differs:", k)
    cases = len({k.rsplit(" ", 1)[0] for k in A})
    print(f"compared {len(A)} outputs of {cases} cases: {len(bad)} differ")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not a.out:
        ap.error("OUT.txt or --compare A B")
    out = Out(a.out)
    poisson_cases(out)
    neighbour_cases(out)
    print(f"wrote {out.outputs} outputs of {out.cases} cases to {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
