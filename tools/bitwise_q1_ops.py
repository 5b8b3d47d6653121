#!/usr/bin/env python3
"""SHA-256 of every output of one seeded case set of the three element-owner-march operators (dn_ns_apply, dn_transport_apply, the 2-D
dn_poisson_coef_grad): one line per output, "<case> <output> <digest>".  Run it once per library (DN_LIB_PATH selects one, one process
each) and compare the two listings: `python tools/bitwise_q1_ops.py --compare A.txt B.txt` prints the differing lines and the counts and
exits 1 if any differ.

Cases: rules of 2, 3, 4 points per axis; every compile-time form the dispatch can reach (NS: MASK / BCF / FGP x forward / VJP; transport:
MASK / BCF / NU / FGP / REACT x forward / VJP with r_first_wins and in_num / in_den; coef-grad: HASV x WANT 1, 2, 3 x no mask / u8 / f32 x
BCF with one and with two conditions); uint8 and fp32 masks, shared and per-sample; the meshes of MESHES (chunk seams at 62 columns,
strip seams, one mesh of 513 x 513).  Outputs: residuals or gradients, sumsq, norm(s).

Usage: python tools/bitwise_q1_ops.py OUT.txt [--meshes 2x2x1,62x9x3,...]
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MESHES = [(2, 2, 1), (62, 9, 3), (63, 17, 2), (64, 5, 1), (125, 33, 2), (513, 513, 4)]     # nx, ny, B
DEV = "cuda:0"


class Seeds:
    def __init__(self, base):
        self.n = base

    def rand(self, shape, lo=-0.5):
        self.n += 1
        g = torch.Generator().manual_seed(self.n)
        return (lo + torch.rand(shape, generator=g)).to(DEV)

    def mask(self, shape, kind, frac=0.15):
        m = self.rand(shape, 0.0) < frac
        return m.to(torch.uint8) if kind == "u8" else m.float()


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


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


def ns_cases(out, ops, geom, tag, nx, ny, B, ngp, sd):
    shape, G = (B, 1, ny, nx), ngp * ngp
    u, v, p = (sd.rand(shape) for _ in range(3))
    cot = tuple(sd.rand(shape) for _ in range(3))
    fgp = {0: None, 1: (sd.rand((B, G, ny - 1, nx - 1)), 0.3), 2: (sd.rand((1, G, ny - 1, nx - 1)), sd.rand((B, G, ny - 1, nx - 1)))}
    masks = {"none": None,
             "A": (sd.mask((1, 1, ny, nx), "u8"), sd.mask(shape, "f32"), None),
             "B": (sd.mask((1, 1, ny, nx), "f32"), sd.mask(shape, "u8"), sd.mask(shape, "f32"))}
    const = (0.3, -0.2, 0.1)
    fields = {"A": (sd.rand(shape), sd.rand((1, 1, ny, nx)), 0.1), "B": (sd.rand((1, 1, ny, nx)), 0.25, sd.rand(shape))}
    num, den = sd.rand(3, 0.5), sd.rand(3, 0.5)
    kw = dict(visco=0.01, wscale=0.37, tau_h=(0.11, 0.07))
    for mk in ("none", "A", "B"):
        for bcf in ((False,) if mk == "none" else (False, True)):
            vals = fields[mk] if bcf else const
            for fk in (0, 1, 2):
                name = f"ns {tag} mask={mk} bcf={int(bcf)} fgp={fk}"
                R, s, n = ops.ns_apply(geom, u, v, p, masks[mk], vals, f_gp=fgp[fk], want_norms=True, **kw)
                out.case(name + " fwd", R0=R[0], R1=R[1], R2=R[2], sumsq=s, norms=n)
                scaled = fk != 1
                g, s, n = ops.ns_apply(geom, u, v, p, masks[mk], vals, f_gp=fgp[fk], cot=cot, want_norms=True,
                                       in_num=num if scaled else None, in_den=den if scaled else None, **kw)
                out.case(name + f" vjp scaled={int(scaled)}", g0=g[0], g1=g[1], g2=g[2], sumsq=s, norms=n)


def transport_cases(out, ops, geom, tag, nx, ny, B, ngp, sd):
    shape, G = (B, 1, ny, nx), ngp * ngp
    u, cot = sd.rand(shape), sd.rand(shape)
    nus = {0: None, 1: sd.rand(shape, 0.5), 2: sd.rand((1, 1, ny, nx), 0.5)}
    fgp = {0: None, 1: sd.rand((B, G, ny - 1, nx - 1)), 2: sd.rand((1, G, ny - 1, nx - 1))}
    masks = {"none": None,
             "A": (sd.mask((1, 1, ny, nx), "u8"), sd.mask(shape, "f32")),
             "B": (sd.mask(shape, "f32", 0.3), sd.mask((1, 1, ny, nx), "u8", 0.3)),
             "one": (sd.mask(shape, "u8"), None)}
    vals = {False: (0.3, -0.2), True: (sd.rand(shape), sd.rand((1, 1, ny, nx)))}
    num, den = sd.rand(1, 0.5), sd.rand(1, 0.5)
    for mk in ("none", "A", "B", "one"):
        for bcf in ((False,) if mk == "none" else (False, True)):
            bv = (vals[bcf][0], 0.0) if mk == "one" else vals[bcf]
            for nk in (0, 1, 2):
                for react in ((0.0, 0.0, 0.0, 0.0), (0.1, 0.5, -0.3, 0.2)):
                    kw = dict(nu=nus[nk], bc=masks[mk], bc_values=bv, r_first_wins=(mk == "B"), adv=(0.7, -0.4), kappa=(0.02, 0.03), tau=0.05,
                              react=react, wscale=0.37)
                    name = f"transport {tag} mask={mk} bcf={int(bcf)} nu={nk} react={int(react[1] != 0)}"
                    for fk in (0, 1, 2):
                        R, s, n = ops.transport_apply(geom, u, f_gp=fgp[fk], want_norm=True, **kw)
                        out.case(name + f" fwd fgp={fk}", R=R, sumsq=s, norm=n)
                    for sc in (0, 1, 2):            # plain, in_num, in_num / in_den
                        g, s, n = ops.transport_apply(geom, u, cot=cot, want_norm=True, in_num=num if sc else None, in_den=den if sc == 2 else None, **kw)
                        out.case(name + f" vjp scale={sc}", g=g, sumsq=s, norm=n)


def coef_grad_cases(out, ops, geom, tag, nx, ny, B, ngp, sd):
    shape = (B, 1, ny, nx)
    u, v = sd.rand(shape), sd.rand(shape)
    sc = sd.rand(1, 0.5)
    for kind in ("none", "u8", "f32"):
        for nbc in ((0,) if kind == "none" else (1, 2)):
            for fields in ((False,) if kind == "none" else (False, True)):
                dl = []
                for k in range(nbc):
                    per_sample = k == 0 if nbc == 2 else fields
                    m = sd.mask(shape if per_sample else (1, 1, ny, nx), kind)
                    val = (sd.rand(shape) if k == 0 else sd.rand((1, 1, ny, nx))) if fields and k == nbc - 1 else 0.3 - 0.5 * k
                    dl.append((m, val))
                for hasv in (False, True):
                    for want in (("nu",), ("f",), ("nu", "f")):
                        gn, gf = ops.poisson_coef_grad(geom, u, v if hasv else None, dl, 0.8, -1.3, 0.37, want=want, in_scale=sc if hasv else None)
                        out.case(f"coef_grad {tag} mask={kind} nbc={nbc} bcf={int(fields)} hasv={int(hasv)} want={'+'.join(want)}", g_nu=gn, g_f=gf)


def run(path, meshes):
    from diffnet_amd import DiffNet2DFEM, ops
    out = Out(path)
    for nx, ny, B in meshes:
        for ngp in (2, 3, 4):
            m = DiffNet2DFEM(None, domain_sizes=(nx, ny), domain_lengths=(1.0, 0.7), domain_size=nx, domain_length=1.0, ngp_1d=ngp).to(DEV)
            tag = f"{nx}x{ny} B={B} ngp={ngp}"
            base = 1000 * (nx * 7 + ny) + 100 * ngp
            ns_cases(out, ops, m.geom, tag, nx, ny, B, ngp, Seeds(base))
            transport_cases(out, ops, m.geom, tag, nx, ny, B, ngp, Seeds(base + 30))
            coef_grad_cases(out, ops, m.geom, tag, nx, ny, B, ngp, Seeds(base + 60))
            torch.cuda.synchronize()
            print(f"{tag}: {out.cases} cases, {out.outputs} outputs so far", flush=True)
    print(f"wrote {out.outputs} outputs of {out.cases} cases to {path}")


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
    ap.add_argument("--meshes", default=",".join(f"{a}x{b}x{c}" for a, b, c in MESHES))
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not a.out:
        ap.error("OUT.txt or --compare A B")
    run(a.out, [tuple(int(x) for x in s.split("x")) for s in a.meshes.split(",")])
    return 0


if __name__ == "__main__":
    sys.exit(main())
