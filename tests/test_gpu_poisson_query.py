"""The invariant that poisson_choose (csrc/poisson_fused.hip) holds in one place: a launch leaves exactly `launched` per-workgroup partial
sums at the front of each of the two partial arrays, the second array starts `stride` doubles behind the first, and the deferred final
reduction reads exactly those.  One PoissonPlan(pipelined_sums=True) -- it owns its workspace -- per kernel family that can defer its
sums (every family but the 3-D Q2 / Q3 one), at the smallest meshes of tools/poisson_dispatch_trace.py: the workspace behind the header is
filled with 0xFF bytes (NaN as doubles), the launch runs, and the entries that are no longer NaN must be 0 .. launched - 1 and
stride .. stride + launched - 1 with `launched` and `stride` as dn_poisson_query answers for the plan's own arguments;
finish_sums() must then give the sums of the in-kernel reduction bit for bit."""
import ctypes as C

import pytest
import torch

from test_gpu_parity import boundary_mask, dev, seeded

pytestmark = pytest.mark.gpu
WS_HEADER = 4160

# (sizes (nx, ny[, nz]), degree, ngp, B, forcing, mask form, switches, family)
CASES = [
    ((64, 64), 1, 2, 1, "nodal", "u8", dict(PLAN2D="128,4,4,4"), "2d_q1_cf"),           # chained strips
    ((65, 65), 1, 2, 1, "nodal", "f32", {}, "2d_q1_cf"),
    ((66, 66), 1, 3, 3, "gp", "u8", {}, "2d_q1_rule"),
    ((130, 37), 1, 2, 3, None, "bits", {}, "2d_q1_cf"),
    ((65, 65), 2, 3, 1, "nodal", "u8", {}, "2d_q23"),
    ((34, 21, 11), 1, 2, 1, "nodal", "box", {}, "3d_q1_cfz"),
    ((34, 21, 11), 1, 2, 3, "nodal", "u8", dict(Q1_3D_N2="1"), "3d_q1_n2"),
    ((34, 16, 9), 1, 2, 1, "nodal", "u8", dict(Q1_3D_E1="1"), "3d_q1_n1"),
    ((33, 33, 33), 1, 2, 1, None, "f32", {}, "3d_q1_t16"),
    ((5, 4, 3), 1, 3, 3, "nodal", "u8", {}, "3d_q1_generic"),
]


@pytest.mark.parametrize("sizes,deg,ngp,B,forcing,mask,sw,family", CASES, ids=[f"{'x'.join(map(str, c[0]))}-{c[-1]}" for c in CASES])
def test_a_launch_leaves_its_partial_sums_where_the_query_says(sizes, deg, ngp, B, forcing, mask, sw, family):
    from diffnet_amd import BoxFaces, PackedMask, _lib, ops
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    geom = FemGeometry(len(sizes), sizes, tuple(1.0 / (n - 1) for n in sizes), deg, ngp, gx, gw)
    shape = (B, 1, *geom.node_shape)
    u, nu = seeded(shape, 11).to(dev()), seeded(shape, 12, 0.5).to(dev())
    f = seeded(shape, 13).to(dev()) if forcing == "nodal" else None
    f_gp = seeded((B, geom.ngp_total, *geom.elem_shape), 14).to(dev()) if forcing == "gp" else None
    img = boundary_mask((1,) + shape[1:]).to(dev())
    cond = {"u8": img.to(torch.uint8), "f32": img, "bits": PackedMask.pack(img), "box": BoxFaces("all")}[mask]
    scale = 1.0 / (B * geom.nelem_total)
    kwargs = dict(alpha=2.0, beta=1.0, c=1.0, wscale=1.0, out_scale=scale, want_out=True, want_sums=True, loss_scale=scale)
    try:
        for k, v in sw.items():
            _lib.config_set(k, v)
        ref = [t.clone() for t in ops.PoissonPlan(geom, u, nu, f, f_gp, [(cond, 0.0)], **kwargs).launch()]
        plan = ops.PoissonPlan(geom, u, nu, f, f_gp, [(cond, 0.0)], pipelined_sums=True, **kwargs)
        kern = _lib.DnPoissonKernel()
        assert _lib.lib().dn_poisson_query(C.byref(plan.mesh), C.byref(plan.args), C.byref(kern)) == 0
        assert _lib.POISSON_FAMILIES[kern.family] == family
        if "PLAN2D" in sw:
            assert kern.W == 4
        ws = next(t for t in plan.keep if isinstance(t, torch.Tensor) and t.data_ptr() == plan.args.workspace)
        assert ws.numel() == plan.args.workspace_bytes >= kern.workspace_bytes == WS_HEADER + 16 * kern.stride
        part = ws[WS_HEADER:WS_HEADER + (ws.numel() - WS_HEADER) // 8 * 8]
        part.fill_(0xFF)
        plan.launch()
        torch.cuda.synchronize()
        written = ~torch.isnan(part.view(torch.float64))
        want = torch.zeros_like(written)
        want[:kern.launched] = True
        want[kern.stride:kern.stride + kern.launched] = True
        assert 0 < kern.launched <= kern.stride
        assert torch.equal(written, want), (kern.launched, kern.stride, torch.nonzero(written != want).flatten()[:8].tolist())
        assert torch.equal(plan.result[0], ref[0])
        plan.finish_sums()
        torch.cuda.synchronize()
        assert torch.equal(plan.result[1], ref[1]), (plan.result[1].tolist(), ref[1].tolist())
        assert torch.equal(plan.result[2], ref[2])
    finally:
        for k in sw:
            _lib.config_set(k, "")
