"""CPU-only checks of the general winding-number operator (dn_winding_field, diffnet_amd/winding.py): the ABI's three statements agree,
every documented bad argument is rejected before a launch, the float64 restatement the GPU tests compare against (tests/winding_ref.py)
reproduces the reference's golden vectors including the swapped axes and equals the existing 2-D oracle in its setting, the derived
error bound has teeth, the inputs of the GPU tests keep their distance from the cloud, the mask inputs are safely classified, and the
wrappers validate their arguments."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import winding_ref as wr

BADARG = -1


def golden():
    z = np.load(os.path.join(GOLDEN, "winding3d_n5_p37.npz"))
    return {k: torch.from_numpy(z[k]) for k in ("q", "points", "normals", "area", "winding64", "winding32")}


def restate_torch(points, normals, area, q, swap=True):
    """compute_winding_torch on the general formula: (1, B, n, n, n), with the reference's swap of the first two grid axes"""
    n = q.shape[-1]
    w, A = wr.winding_general(points, normals, area[..., 0], q[0].reshape(3, -1), "l1", 3, 1.0)
    w, A = (t.reshape(1, points.shape[0], n, n, n) for t in (w, A))
    return (w.transpose(2, 3), A.transpose(2, 3)) if swap else (w, A)


def test_winding_field_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    header = open(os.path.join(ROOT, "include", "diffnet_hip.h")).read()
    for s in ("dn_winding_field", "dn_winding_field_tile"):
        assert hasattr(h, s) and s in _lib.SYMBOLS and f"int {s}(" in header, s
    decl = re.search(r"int dn_winding_field\((.*?)\);", header, flags=re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["points", "normals", "area", "queries", "out", "mask", "batch", "npts", "nq", "dim",
                                                         "metric", "power", "scale", "threshold", "tile", "stream"]
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    want = [C.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
    assert _lib.SYMBOLS["dn_winding_field"] == (C.c_int, want)
    assert h.dn_abi_version() == _lib.ABI_VERSION
    assert "winding_field.hip" in build.SOURCES and "winding.hip" in build.SOURCES
    from diffnet_amd import ops
    # the tiles the Python side offers are the ones the library accepts and picks from
    assert ops.WINDING_TILES == wr.TILES and ops.WINDING_CHUNK == wr.CHUNK and ops.WINDING_THREADS == wr.THREADS
    for B, nq in ((1, 1), (1, 25 ** 3), (1, 128 ** 3), (16, 512 ** 2), (2, 300000), (3, 200000)):
        assert h.dn_winding_field_tile(B, nq) in ops.WINDING_TILES
    assert h.dn_winding_field_tile(1, 25 ** 3) == 1 and h.dn_winding_field_tile(1, 128 ** 3) == 4 and h.dn_winding_field_tile(2, 300000) == 2
    assert h.dn_winding_field_tile(0, 5) == BADARG and h.dn_winding_field_tile(1, 0) == BADARG


def test_winding_field_rejects_bad_arguments_before_touching_the_gpu():
    """every argument the header lists returns DN_E_BADARG without a launch (so this runs without a GPU); the pointers are never read"""
    from diffnet_amd import _lib
    L = _lib.lib()
    p = 4096                                            # a non-null address: validation never dereferences it
    good = dict(points=p, normals=p, area=p, queries=p, out=p, mask=p, batch=2, npts=10, nq=100, dim=3, metric=0, power=3, scale=1.0,
                threshold=0.5, tile=0, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.dn_winding_field(*(a[k] for k in good))

    for name in ("points", "normals", "queries"):
        assert call(**{name: None}) == BADARG, name
    assert call(out=None, mask=None) == BADARG
    for bad in (1, 4, 0, -3):
        assert call(dim=bad) == BADARG, bad
    for bad in (1, 4, 0):
        assert call(power=bad) == BADARG, bad
    for bad in (2, -1):
        assert call(metric=bad) == BADARG, bad
    for bad in (3, 8, -1, 16):
        assert call(tile=bad) == BADARG, bad
    for bad in (0, -1, 65536):
        assert call(batch=bad) == BADARG, bad
    assert call(npts=0) == BADARG and call(npts=-5) == BADARG
    assert call(nq=0) == BADARG and call(nq=-1) == BADARG
    # the grid holds 16777215 workgroups of 256 * tile queries
    for tile in (1, 2, 4):
        assert call(nq=16777215 * 256 * tile + 1, tile=tile) == BADARG, tile
    assert call(nq=1 << 40) == BADARG


def test_restatement_reproduces_the_reference_golden_with_its_swapped_axes():
    g = golden()
    args64 = [g[k].double() for k in ("points", "normals", "area", "q")]
    w, A = restate_torch(*args64)
    assert w.shape == g["winding64"].shape == (1, 2, 5, 5, 5)
    # float64 against float64: the two differ by the order of a 37-term sum and of the products
    err = float(((w - g["winding64"]).abs() / A).max())
    print(f"float64 restatement against the reference's float64 result: max |diff| / A = {err:.3g}")
    assert err <= 64 * 2.0 ** -53
    # the reference's own float32 result is within the bound the GPU kernel is held to
    n = wr.n_roundings(37, 3, "l1", 3)
    r32 = wr.bound_ratio(g["winding32"], w, A, n)
    print(f"the reference's float32 result: {r32:.3g} x the bound")
    assert r32 <= 1.0
    plain, _ = restate_torch(*args64, swap=False)
    r = wr.bound_ratio(plain, w, A, n)
    print(f"unswapped axes: {r:.3g} x the bound")
    assert r > 1e3


def test_restatement_equals_the_2d_oracle_in_its_setting():
    from oracle.fem_oracle import winding_nodes
    z = np.load(os.path.join(GOLDEN, "winding_n17_p40.npz"))
    pts, nrm, nodes = (torch.from_numpy(z[k]).double() for k in ("points", "normals", "nodes"))
    ref = winding_nodes(pts, nrm, nodes)                                        # (B, 1, nx, ny)
    w, A = wr.winding_general(pts, nrm, None, nodes.reshape(2, -1), "l1", 3, (4.0 * math.pi) ** -3)
    B, ny, nx = pts.shape[0], nodes.shape[1], nodes.shape[2]
    w, A = (t.reshape(B, 1, ny, nx).transpose(2, 3) for t in (w, A))
    assert w.shape == ref.shape
    assert float(((w - ref).abs() / A).max()) <= 64 * 2.0 ** -53
    np.testing.assert_allclose(w.numpy(), z["winding"], rtol=2e-4, atol=1e-5 * np.abs(z["winding"]).max())


TEETH = [("3d_l1_p3_area", 2, 257, 517), ("2d_l1_p2_area", 3, 256, 257), ("3d_l2_p3", 2, 255, 300), ("2d_l2_p2", 1, 513, 255)]


@pytest.mark.parametrize("name,B,npts,nq", TEETH, ids=[t[0] for t in TEETH])
def test_bound_passes_float32_and_rejects_wrong_formulas(name, B, npts, nq):
    p = wr.problem(name, B, npts, nq)
    dim = p["points"].shape[-1]
    pts, nrm, area, qs = p["points"].double(), p["normals"].double(), p["area"].double(), p["queries"].double()
    w32, _ = wr.winding_general(p["points"], p["normals"], p["area"], p["queries"], p["metric"], p["power"], p["scale"])
    ok = wr.bound_ratio(w32, p["ref"], p["A"], p["n"])
    other = {"l1": "l2", "l2": "l1"}[p["metric"]]
    swapped = qs[[1, 0] + list(range(2, dim))]
    bad = {"area dropped": wr.winding_general(pts, nrm, None, qs, p["metric"], p["power"], p["scale"] * float(p["area"].mean()))[0],
           "other power": wr.winding_general(pts, nrm, area, qs, p["metric"], 5 - p["power"], p["scale"])[0],
           "other metric": wr.winding_general(pts, nrm, area, qs, other, p["power"], p["scale"])[0],
           "query axes exchanged": wr.winding_general(pts, nrm, area, swapped, p["metric"], p["power"], p["scale"])[0]}
    bad = {k: wr.bound_ratio(v, p["ref"], p["A"], p["n"]) for k, v in bad.items()}
    print(f"float32 torch evaluation: {ok:.3g} x the bound; float64 evaluations of the wrong formula:", {k: f"{v:.3g}" for k, v in bad.items()})
    assert ok <= 1.0
    for k, v in bad.items():
        assert v > 1.0, f"{k}: the bound does not notice ({v:.3g})"


@pytest.mark.parametrize("tile", wr.TILES)
@pytest.mark.parametrize("name", list(wr.PARAMS))
def test_gpu_cases_keep_points_off_the_queries(name, tile):
    for B, npts, nq in wr.seam_cases(tile):
        p = wr.problem(name, B, npts, nq)
        assert p["l1min"] >= wr.MIN_L1, (name, B, npts, nq, p["l1min"])
        assert torch.allclose(torch.linalg.vector_norm(p["normals"], dim=-1), torch.ones(B, npts), atol=1e-6)
        assert bool((p["A"] > 0).all()) and bool(torch.isfinite(p["ref"]).all())
        if p["area"] is not None and npts > 1:
            assert float(p["area"].std()) > 0 and (B == 1 or not torch.equal(p["area"][0], p["area"][1]))
    assert {c[1] for c in wr.seam_cases(tile)} == {1, wr.CHUNK - 1, wr.CHUNK, wr.CHUNK + 1, 2 * wr.CHUNK + 1}
    W = wr.THREADS * tile
    assert {c[2] for c in wr.seam_cases(tile)} == {1, W - 1, W + 1, 3 * W + 5} and {c[0] for c in wr.seam_cases(tile)} == {1, 2, 3}


@pytest.mark.parametrize("n", [9, 17])
def test_mask_inputs_are_classified_with_a_wide_margin(n):
    """the Fibonacci sphere of 1000 points, radius 0.3: the float64 true winding number stays 0.247 away from the threshold on every
    node and classifies every node as the geometry does, so the GPU mask must equal the geometric inside exactly"""
    s = wr.sphere_problem(n)
    margin = float((s["w"] - 0.5).abs().min())
    print(f"{n}^3 nodes: min |w - 0.5| = {margin:.4f}; w in [{float(s['w'].min()):.4f}, {float(s['w'].max()):.4f}]")
    assert margin >= 0.247 - 5e-4
    assert torch.equal(s["w"] > 0.5, s["inside"])
    assert 0 < int(s["inside"].sum()) < n ** 3
    # the error bound of the kernel is orders of magnitude below that margin: no node may be excluded
    assert float((s["n"] * wr.U * s["A"]).max()) < 1e-3 * margin


def test_read_xyzna_round_trip(tmp_path):
    from diffnet_amd.winding import read_xyzna
    pts = np.array([[0.1, -0.2, 0.3], [1.5, 2.5e-3, -3.25], [7.0, 8.0, 9.0]])
    nrm = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.6, 0.0, 0.8]])
    area = np.array([[0.25], [1e-3], [2.0]])
    path = tmp_path / "three.xyzna"
    with open(path, "w") as fh:
        fh.write("3\n")
        for row in list(pts) + list(nrm) + list(area):
            fh.write(" ".join(repr(float(v)) for v in row) + "\n")
    p, n, a = read_xyzna(str(path))
    assert p.shape == (3, 3) and n.shape == (3, 3) and a.shape == (3, 1)
    assert np.array_equal(p, pts) and np.array_equal(n, nrm) and np.array_equal(a, area)
    with open(path, "w") as fh:
        fh.write("3\n0 0 0\n")
    with pytest.raises(ValueError):
        read_xyzna(str(path))


def test_wrappers_validate_their_arguments():
    from diffnet_amd import ops, winding
    from diffnet_amd._lib import DiffNetHipError
    g = golden()
    pts, nrm, area, q = g["points"], g["normals"], g["area"], g["q"]
    with pytest.raises(ValueError, match="cubic"):
        winding.compute_winding_torch(pts, nrm, area, torch.zeros(1, 3, 5, 5, 6))
    with pytest.raises(ValueError, match="batch 1"):
        winding.compute_winding_torch(pts, nrm, area, torch.zeros(2, 3, 5, 5, 5))
    with pytest.raises(ValueError):
        winding.compute_winding_torch(pts, nrm, area, q[0])
    with pytest.raises(ValueError):
        winding.compute_winding_torch(pts, nrm[:, :30], area, q)
    with pytest.raises(ValueError):
        winding.compute_winding_torch(pts, nrm, area[:, :30], q)
    with pytest.raises(TypeError, match="float32"):
        winding.compute_winding_torch(pts.double(), nrm, area, q)
    with pytest.raises(TypeError, match="float32"):
        winding.compute_winding_torch(pts, nrm, area, q.double())
    with pytest.raises(TypeError, match="float32"):
        winding.winding_number(pts, nrm.half(), area, q[0])
    with pytest.raises(ValueError, match="queries"):
        winding.winding_number(pts, nrm, area, q[0, :2])                        # 2-D queries for 3-D points
    with pytest.raises(ValueError):
        winding.winding_mask(pts, nrm, area, q[0], metric="linf")
    with pytest.raises(TypeError):
        winding.winding_mask(pts, nrm, area, q[0], dtype=torch.int32)
    # mismatched devices: a cloud on another device than its normals (the meta device stands in for a second GPU)
    with pytest.raises(ValueError, match="is on"):
        winding.winding_number(pts, nrm.to("meta"), area, q[0])
    with pytest.raises(ValueError, match="is on"):
        ops.winding_field(pts, nrm, area[..., 0].contiguous().to("meta"), q[0].reshape(3, -1))
    # everything on the host: no CPU fallback
    with pytest.raises(DiffNetHipError):
        winding.compute_winding_torch(pts, nrm, area, q)
    with pytest.raises(DiffNetHipError):
        winding.winding_mask(pts, nrm, None, q[0])
    for kw in (dict(metric="l3"), dict(power=4), dict(tile=3), dict(want_field=False)):
        with pytest.raises(ValueError):
            ops.winding_field(pts, nrm, None, q[0].reshape(3, -1), **kw)
    with pytest.raises(ValueError, match="contiguous"):
        ops.winding_field(pts.transpose(0, 1).contiguous().transpose(0, 1), nrm, None, q[0].reshape(3, -1))
