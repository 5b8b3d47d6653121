#!/usr/bin/env python3
"""Golden vectors of the 3-D stabilised eikonal residual loss from the *imported* reference script.

Like tools/gen_golden_eikonal.py (whose approach and shims it reuses), this runs only where the reference repository is present.  It
imports examples/eiqonal/single_instance/05_3d_sphere_loss4.py as a module and calls its own loss body, Eiqonal.loss4, unbound, on
objects built by the library constructor.  Only data -- inputs and the reference's outputs -- is written, to
tests/golden/loss_eikonal3d_*.npz, batch 1.

  loss_eikonal3d_sphere_n9.npz       9^3 nodes, ngp 2, tau 0.25
  loss_eikonal3d_sphere_n7_g3.npz    7^3 nodes, ngp 3, tau 0.25

The body calls `self.bf_1d_th` and `self.bf_1d_der_th`, which the reference library does not define: the generator sets them on the
object, as the linear 1-D basis (1 -+ x) / 2 and its derivative.  And the body adds two point-cloud terms to the loss; they get
neutral inputs: ONE point strictly inside a diagonal element ((k + 0.4) h on all three axes), u exactly 0 on the 3 x 3 x 3 nodes around
that element and zero normals.  Then the reconstruction term is exactly 0 and the normals term exactly (0 - 1)^2 = 1, both with zero
gradient.  The file's `loss` is ||R||_F + point_terms and `grad` the gradient of ||R||_F.  The generator asserts this from the R1 the
body leaves in `self.domain_loss`, which is stored too.

Elsewhere u is the distance to a sphere of radius 0.3 plus seeded noise of amplitude h / 2, so that |grad u| = O(1) and the terms
tau u grad u, |grad u|^2 and -1 have comparable size.

Each file holds: kwargs, script, u, pc (the point), tau, sq, wscale, R1 (nz, ny, nx), point_terms (the constant 1), the reference's
`loss` and its `grad` with respect to u (autograd through the reference's own body).

Usage: python tools/gen_golden_eikonal3d.py [--out tests/golden]
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import T, install_shims, load_script, make, rng  # noqa: E402

SCRIPT = "examples/eiqonal/single_instance/05_3d_sphere_loss4.py"

PROVENANCE = """loss_eikonal3d_*.npz: written by tools/gen_golden_eikonal3d.py from the reference's own loss body, called unbound:
  loss_eikonal3d_sphere_n9.npz       examples/eiqonal/single_instance/05_3d_sphere_loss4.py::Eiqonal.loss4, 9^3 nodes, ngp 2, tau 0.25
  loss_eikonal3d_sphere_n7_g3.npz    the same body, 7^3 nodes, ngp 3, tau 0.25
Data only: u (distance to a sphere of radius 0.3 + seeded noise of amplitude h/2, exactly 0 on the 3 x 3 x 3 nodes around the point's
element), the one neutral point, the reference's loss (= ||R1||_F + point_terms: the point-cloud terms are exactly 0 and 1), its
gradient and R1.  bf_1d_th / bf_1d_der_th, which the body calls and the reference library does not define, were set by the generator
to the linear 1-D basis (1 -+ x) / 2 and its derivative.
"""


def field(n, h, k, seed):
    """distance to a sphere + noise of amplitude h / 2; exactly 0 on the nodes k .. k + 2 of all three axes (the point's element is (k, k, k))"""
    g = rng(seed)
    x = torch.linspace(0.0, 1.0, n)
    r = torch.sqrt((x[None, None, :] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[:, None, None] - 0.5) ** 2)
    u = r - 0.3 + 0.5 * h * (2.0 * torch.rand((n, n, n), generator=g) - 1.0)
    u[k:k + 3, k:k + 3, k:k + 3] = 0.0
    return u.reshape(1, 1, n, n, n).float()


def run_case(outdir, tag, fn, m, kw, inputs, pc, u):
    m.bf_1d_th = lambda x: torch.stack((0.5 * (1.0 - x), 0.5 * (1.0 + x)))
    m.bf_1d_der_th = lambda x: torch.stack((-0.5 * torch.ones_like(x), 0.5 * torch.ones_like(x)))
    ur = u.clone().requires_grad_(True)
    with contextlib.redirect_stdout(io.StringIO()):
        loss = fn(m, ur, inputs, torch.ones_like(u))
    grad, = torch.autograd.grad(loss, ur)
    R1 = m.domain_loss.reshape(u.shape[-3:])
    nrm = torch.norm(R1)
    # the point terms are exactly 0 + 1 (that they pass no gradient: tests/test_eikonal3d_host.py, against the gradient of ||R||_F alone)
    c = float(round(float(loss.detach()) - float(nrm)))
    assert c == 1.0 and float(loss.detach()) == float((nrm + 0.0) + c), (tag, float(loss.detach()), float(nrm))
    tau = float(m.tau)
    out = dict(kwargs=repr(kw), script=SCRIPT + "::Eiqonal.loss4", u=T(u), pc=np.asarray(pc, dtype=np.float32), tau=np.float64(tau),
               sq=np.float64(1.0 + tau), wscale=np.float64((0.5 * m.h) ** 3), R1=T(R1), point_terms=np.float32(c), loss=np.float32(T(loss)),
               grad=T(grad))
    np.savez_compressed(os.path.join(outdir, f"loss_eikonal3d_{tag}.npz"), **out)
    print("eikonal3d", tag, "loss", float(loss.detach()), "point terms", c, "||R1||", float(nrm), "max|grad|", float(grad.abs().max()))


def gen(outdir):
    from DiffNet.DiffNetFEM import DiffNet3DFEM
    mod = load_script(SCRIPT, "ref_eik3d_sphere")

    for tag, n, ngp, seed in (("sphere_n9", 9, 2, 95), ("sphere_n7_g3", 7, 3, 97)):
        kw = dict(domain_size=n, nsd=3) if ngp == 2 else dict(domain_size=n, nsd=3, ngp_1d=ngp)
        m = make(mod.Eiqonal, DiffNet3DFEM, **kw)
        m.tau = 0.25                                   # what the script's __init__ sets
        h = float(m.h)
        k = n // 2 - 1
        p = (k + 0.4) * h                              # strictly inside element (k, k, k)
        assert int(np.float32(p) / np.float32(m.hx)) == k
        u = field(n, h, k, seed)
        # inputs (1, 2, Npts, 3) = points, normals
        inputs = torch.tensor([[p, p, p], [0.0, 0.0, 0.0]]).reshape(1, 2, 1, 3)
        run_case(outdir, tag, mod.Eiqonal.loss4, m, kw, inputs, (p, p, p), u)
    with open(os.path.join(outdir, "PROVENANCE_eikonal3d.txt"), "w") as fh:
        fh.write(PROVENANCE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    install_shims()
    torch.manual_seed(0)
    gen(a.out)


if __name__ == "__main__":
    main()
