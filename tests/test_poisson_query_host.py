"""The launch plan of dn_poisson_apply, asked of the library on the host (dn_poisson_query calls poisson_choose, the function the launch, the
deferred final reduction and a folding launch call): one written-out table of calls that reaches every kernel family, the invariants that
tie a launch's partial sums to the workspace layout, and the Python predicate of `_auto_pack` / `_fused` held equal to the query.  No GPU:
the query follows no pointer, so the arguments carry made-up addresses."""
import contextlib
import ctypes as C

import pytest

BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
WS_HEADER = 4160
ADDR = 0x7F0000000000                    # made-up device addresses, 4 KiB apart: only NULL-ness and alignment are looked at
FAMILIES = ["2d_q1_cf", "2d_q1_rule", "2d_q23", "3d_q1_n1", "3d_q1_t16", "3d_q1_generic", "3d_q1_n2", "3d_q1_cfz", "3d_q23"]
SWITCHES = ("Q1_RULE_KERNEL", "Q1_3D_T16", "Q1_3D_E1", "Q1_3D_N2", "Q1_3D_E1SUM", "PLAN2D", "PLAN3D")


@contextlib.contextmanager
def switches(**kw):
    from diffnet_amd import _lib
    assert all(_lib.config_get(k) == "" for k in SWITCHES)
    try:
        for k, v in kw.items():
            _lib.config_set(k, v)
        yield
    finally:
        for k in kw:
            _lib.config_set(k, "")


def mesh_of(sizes, deg=1, ngp=2, B=1):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    return FemGeometry(len(sizes), sizes, tuple(1.0 / (n - 1) for n in sizes), deg, ngp, gx, gw).mesh_struct(B)


def args_of(mesh, nu=False, f=None, bc=(), sums=True, out=True, strip_select=0, fold=False, defer=False, alpha=2.0, off=0):
    """f: None | "nodal" | "gp" | "load";  bc: up to two of "u8" | "f32" | "field" (fp32 image + value field) | "bits" | "box";  off: bytes
    added to the address of u (a misaligned view)."""
    from diffnet_amd import _lib
    a = _lib.DnPoissonArgs()
    slot = iter(range(1, 32))
    addr = lambda: ADDR + 4096 * next(slot)
    a.u = addr() + off
    a.alpha, a.beta, a.c, a.wscale, a.out_scale = alpha, 1.0, 0.5 * alpha, 1.0, 1.0
    if nu:
        a.nu, a.nu_batched = addr(), 1
    if f in ("nodal", "load"):
        a.f, a.f_batched, a.f_is_load = addr(), 1, int(f == "load")
    elif f == "gp":
        a.f_gp, a.f_batched = addr(), 1
    for k, kind in enumerate(bc):
        d = a.bc[k]
        if kind == "box":
            d.mask_kind, d.box_faces = _lib.MASK_BOX, 0x0F if mesh.nsd == 2 else 0x3F
            continue
        d.mask, d.mask_batched = addr(), 1
        d.mask_kind = {"u8": _lib.MASK_U8, "f32": _lib.MASK_F32, "field": _lib.MASK_F32, "bits": _lib.MASK_BITS}[kind]
        if kind == "field":
            d.field, d.field_batched = addr(), 1
        if kind == "bits":
            d.row_words = (mesh.nx + 31) // 32
    if out:
        a.out = addr()
    if sums or (mesh.nsd == 3 and mesh.degree > 1):
        a.workspace, a.workspace_bytes = addr(), _lib.lib().dn_poisson_workspace_bytes(C.byref(mesh))
    if sums:
        a.energy = addr()
        a.sumsq = a.energy + 8
    a.strip_select, a.defer_sums = strip_select, int(defer)
    keep = None
    if fold:                               # an earlier deferred evaluation of the same call, in a workspace of its own
        keep = args_of(mesh, nu=nu, f=f, bc=bc, defer=True, alpha=alpha)[0]
        keep.workspace += 1 << 30
        a.fold_prev = C.addressof(keep)
    return a, keep


def query(mesh, **kw):
    from diffnet_amd import _lib
    a, keep = args_of(mesh, **kw)
    k = _lib.DnPoissonKernel()
    rc = _lib.lib().dn_poisson_query(C.byref(mesh), C.byref(a), C.byref(k))
    return rc, k


# (sizes (nx, ny[, nz]), mesh keywords, argument keywords, switches, expected family or DN_E_* code)
TABLE = [
    # ---- 2-D
    ((64, 64), {}, {}, {}, "2d_q1_cf"),
    ((64, 64), dict(B=3), dict(nu=True, f="nodal", bc=("u8",)), {}, "2d_q1_cf"),
    ((65, 65), {}, dict(bc=("f32", "u8")), {}, "2d_q1_cf"),
    ((66, 66), dict(ngp=3), dict(bc=("field",)), {}, "2d_q1_cf"),
    ((72, 45), dict(B=3), dict(bc=("bits",)), {}, "2d_q1_cf"),
    ((130, 37), {}, dict(bc=("box", "bits")), {}, "2d_q1_cf"),
    ((97, 97), dict(ngp=4), dict(off=4), {}, "2d_q1_cf"),
    ((325, 33), {}, dict(f="nodal"), {}, "2d_q1_cf"),                                   # the 4 k + 1 form on unaligned vector rows
    ((512, 512), dict(B=3), dict(bc=("bits",), fold=True, defer=True), {}, "2d_q1_cf"),  # chained strips
    ((512, 512), dict(B=3), dict(strip_select=1), {}, "2d_q1_cf"),
    ((64, 64), {}, dict(sums=False), {}, "2d_q1_cf"),
    ((64, 64), {}, dict(f="gp"), {}, "2d_q1_rule"),
    ((65, 65), dict(ngp=3, B=3), dict(f="gp", bc=("u8",)), {}, "2d_q1_rule"),
    ((64, 64), dict(ngp=4), dict(f="nodal"), dict(Q1_RULE_KERNEL="1"), "2d_q1_rule"),
    ((65, 65), dict(deg=2, ngp=3), dict(bc=("f32",)), {}, "2d_q23"),
    ((64, 64), dict(deg=3, ngp=4, B=3), dict(f="gp"), {}, "2d_q23"),
    ((64, 64), {}, dict(bc=("bits",)), dict(Q1_RULE_KERNEL="1"), UNSUPPORTED),
    ((64, 64), {}, dict(bc=("bits", "u8")), {}, UNSUPPORTED),                           # compact conditions beside an image
    ((64, 64), {}, dict(f="gp", bc=("box",)), {}, UNSUPPORTED),
    ((65, 65), dict(deg=2, ngp=3), dict(bc=("box",)), {}, UNSUPPORTED),
    ((64, 64), {}, dict(f="load"), {}, UNSUPPORTED),
    ((65, 65), dict(deg=2, ngp=3), dict(fold=True), {}, UNSUPPORTED),
    ((65, 65), dict(deg=2, ngp=2), {}, {}, UNSUPPORTED),
    ((64, 64), {}, dict(sums=False, out=False), {}, BADARG),
    ((64, 64), {}, dict(strip_select=3), {}, BADARG),
    # ---- 3-D
    ((34, 34, 34), {}, {}, {}, "3d_q1_cfz"),
    ((34, 21, 11), dict(B=3), dict(nu=True, f="nodal", bc=("u8", "u8")), {}, "3d_q1_cfz"),
    ((34, 21, 11), {}, dict(bc=("box", "f32")), {}, "3d_q1_cfz"),
    ((34, 34, 34), {}, dict(f="load", fold=True, defer=True), {}, "3d_q1_cfz"),
    ((34, 34, 34), {}, dict(alpha=0.0), {}, "3d_q1_n2"),                                # no stiffness part
    ((34, 21, 11), {}, dict(bc=("box",)), dict(Q1_3D_N2="1"), "3d_q1_n2"),
    ((34, 34, 34), {}, dict(f="nodal"), dict(Q1_3D_E1SUM="1"), "3d_q1_n2"),
    ((34, 16, 9), {}, dict(bc=("u8",)), dict(Q1_3D_E1="1"), "3d_q1_n1"),
    ((34, 34, 34), {}, dict(bc=("u8",)), dict(Q1_3D_E1="1"), "3d_q1_t16"),                # ny = 34: the one-element plan takes tiles 12 rows high
    ((34, 34, 34), {}, dict(bc=("u8", "f32")), {}, "3d_q1_t16"),                        # images of two kinds: no node-owner form
    ((34, 16, 9), {}, dict(off=4), {}, "3d_q1_n1"),                                     # node pairs not 8-byte aligned
    ((34, 34, 34), {}, {}, dict(Q1_3D_T16="1"), "3d_q1_t16"),
    ((33, 33, 33), dict(B=3), dict(bc=("f32",)), {}, "3d_q1_t16"),                      # odd nx; the plan takes tiles 12 rows high
    ((33, 16, 9), {}, dict(bc=("f32", "f32")), {}, "3d_q1_n1"),
    ((33, 16, 9), {}, dict(bc=("field",)), {}, "3d_q1_t16"),
    ((33, 16, 9), {}, dict(f="gp"), {}, "3d_q1_t16"),
    ((17, 17, 17), dict(ngp=3), dict(f="nodal"), {}, "3d_q1_generic"),                  # larger rules: any tile shape, here 26 x 9
    ((16, 16, 9), dict(ngp=3), dict(f="nodal", bc=("u8",)), {}, "3d_q1_n1"),
    ((16, 16, 9), dict(ngp=4), dict(f="gp"), {}, "3d_q1_t16"),
    ((5, 4, 3), dict(ngp=3), {}, {}, "3d_q1_generic"),
    ((6, 5, 3), {}, dict(strip_select=2), {}, "3d_q1_cfz"),                             # one strip: nothing left for the second launch
    ((34, 34, 34), {}, {}, dict(PLAN3D="32,8,1,5"), "3d_q1_generic"),
    ((9, 7, 5), dict(deg=2, ngp=3, B=2), dict(f="gp", bc=("u8",)), {}, "3d_q23"),
    ((7, 7, 7), dict(deg=3, ngp=4), dict(sums=False), {}, "3d_q23"),
    ((34, 34, 34), {}, dict(bc=("bits",)), {}, UNSUPPORTED),                            # no bit arrays in 3-D
    ((33, 33, 33), {}, dict(bc=("box",)), {}, UNSUPPORTED),
    ((34, 34, 34), {}, dict(bc=("box",)), dict(Q1_3D_E1="1"), UNSUPPORTED),
    ((33, 33, 33), {}, dict(f="load"), {}, UNSUPPORTED),
    ((34, 34, 34), dict(ngp=3), dict(fold=True), {}, UNSUPPORTED),
    ((9, 7, 5), dict(deg=2, ngp=3), dict(strip_select=1), {}, UNSUPPORTED),
    ((9, 7, 5), dict(deg=2, ngp=3), dict(fold=True), {}, BADARG),
]


def run_table():
    from diffnet_amd import _lib
    for sizes, mkw, akw, sw, want in TABLE:
        mesh = mesh_of(sizes, **mkw)
        with switches(**sw):
            rc, k = query(mesh, **akw)
            ws_all = _lib.lib().dn_poisson_workspace_bytes(C.byref(mesh))
        yield (sizes, mkw, akw, sw), mesh, rc, k, want, ws_all


def test_the_table_reaches_every_family_and_every_refusal_is_the_expected_one():
    from diffnet_amd import _lib
    assert sorted(_lib.POISSON_FAMILIES.values()) == sorted(FAMILIES)
    seen = set()
    for row, mesh, rc, k, want, _ in run_table():
        if isinstance(want, int):
            assert rc == want, (row, rc, _lib.POISSON_FAMILIES.get(k.family))
        else:
            assert rc == 0 and _lib.POISSON_FAMILIES[k.family] == want, (row, rc, _lib.POISSON_FAMILIES.get(k.family))
            seen.add(want)
    assert seen == set(FAMILIES)


def test_partial_sums_fit_the_layout_and_the_layout_fits_the_workspace():
    n = 0
    for row, mesh, rc, k, want, ws_all in run_table():
        if rc != 0:
            continue
        n += 1
        assert 0 <= k.launched <= k.stride, (row, k.launched, k.stride)
        assert WS_HEADER + 16 * k.stride <= ws_all and k.workspace_bytes <= ws_all, (row, k.stride, k.workspace_bytes, ws_all)
        if k.family != 9:
            assert k.launched == k.chunks * k.tiles * -(-k.launched_strips // k.W) * mesh.batch, row
            assert tuple(k.tile) == ((k.tile[0], 0) if mesh.nsd == 2 else (k.tile[0], k.tile[1])) and k.tile[0] * max(k.tile[1], 1) <= 256
    assert n == sum(not isinstance(r[-1], int) for r in TABLE)


def test_the_two_halves_of_a_split_evaluation_leave_as_many_partials_as_the_whole():
    n = 0
    for sizes, mkw, akw, sw, want in TABLE:
        if isinstance(want, int) or want == "3d_q23":
            continue
        mesh = mesh_of(sizes, **mkw)
        akw = {k: v for k, v in akw.items() if k != "strip_select"}
        with switches(**sw):
            (rc0, k0), (rc1, k1), (rc2, k2) = (query(mesh, strip_select=s, **akw) for s in (0, 1, 2))
        assert rc0 == rc1 == rc2 == 0, (sizes, akw)
        assert k1.W == 1 and k2.W == 1                                      # a split evaluation selects whole strips: no chains
        assert (k1.R, k1.strips, k1.chunks, k1.tiles) == (k2.R, k2.strips, k2.chunks, k2.tiles)      # the two halves agree on the strips
        assert k1.launched_strips == min(k1.strips, 2) and k2.launched_strips == max(k1.strips - 2, 0)
        if k0.W == 1:
            assert (k1.R, k1.strips, k1.chunks) == (k0.R, k0.strips, k0.chunks)
            assert k1.launched + k2.launched == k0.launched, (sizes, akw)
            n += 1
    assert n >= 20


def test_chained_strips_and_the_unaligned_form_show_in_the_query():
    with switches():
        rc, k = query(mesh_of((512, 512), B=3))
        assert rc == 0 and k.W == 4 and k.R < 16 and k.tile[0] == 128 and k.E == 4 and k.vec == 1
        assert k.launched == k.chunks * -(-k.strips // 4) * 3
        rc, k = query(mesh_of((325, 33)))
        assert rc == 0 and k.ua == 1 and k.E == 4 and k.W == 1
        rc, k = query(mesh_of((325, 33)), f="gp")
        assert rc == 0 and k.ua == 0 and k.E == 2
    with switches(PLAN2D="128,4,4,4"):
        assert query(mesh_of((512, 512)))[1].W == 4
        assert query(mesh_of((512, 512)), strip_select=1)[1].W == 1
        assert query(mesh_of((512, 512)), f="gp")[1].W == 1                 # the override asks for chains where they do not exist


@pytest.mark.parametrize("R", [3, 8])
def test_a_plan3d_override_to_one_element_keeps_the_two_element_form_where_only_it_has_the_path(R):
    """Box faces, a fold and a load vector have no one-element path (the override dropped the faces and the fold)."""
    mesh = mesh_of((34, 34, 34))
    with switches(PLAN3D=f"16,16,1,{R}"):
        rc, k = query(mesh)
        assert rc == 0 and k.E == 1 and k.R == R and k.family == 4
        for akw in (dict(bc=("box",)), dict(bc=("box", "u8")), dict(fold=True), dict(f="load"), dict(f="load", bc=("box",), fold=True)):
            rc, k = query(mesh, **akw)
            assert rc == 0 and k.E == 2 and tuple(k.tile) == (16, 16) and k.family in (7, 8), (akw, rc, k.E, k.family)
    with switches(PLAN3D=f"16,16,2,{R}"):
        rc, k = query(mesh, bc=("box",))
        assert rc == 0 and k.E == 2 and k.R == R


def test_compact_conditions_are_refused_where_no_kernel_reads_them():
    with switches():
        assert query(mesh_of((34, 34, 34)), bc=("bits",))[0] == UNSUPPORTED
        assert query(mesh_of((34, 34, 34)), bc=("box", "bits"))[0] == UNSUPPORTED
        assert query(mesh_of((64, 64)), bc=("box", "f32"))[0] == UNSUPPORTED
        assert query(mesh_of((64, 64)), bc=("u8", "bits"))[0] == UNSUPPORTED
        assert query(mesh_of((64, 64)), f="gp", bc=("bits",))[0] == UNSUPPORTED
        assert query(mesh_of((34, 34, 34)), f="gp", bc=("box",))[0] == UNSUPPORTED
        rc, k = query(mesh_of((64, 64)), bc=("box", "bits"))
        assert rc == 0 and k.compact == 2
        rc, k = query(mesh_of((34, 34, 34)), bc=("box", "u8"))
        assert rc == 0 and k.compact == 1


def test_query_validates_like_the_launch():
    from diffnet_amd import _lib
    h = _lib.lib()
    mesh = mesh_of((64, 64))
    a, _ = args_of(mesh)
    k = _lib.DnPoissonKernel()
    assert h.dn_poisson_query(C.byref(mesh), C.byref(a), None) == BADARG
    assert h.dn_poisson_query(None, C.byref(a), C.byref(k)) == BADARG and h.dn_poisson_query(C.byref(mesh), None, C.byref(k)) == BADARG
    a.workspace_bytes = WS_HEADER
    assert h.dn_poisson_query(C.byref(mesh), C.byref(a), C.byref(k)) == WORKSPACE
    assert k.workspace_bytes == WS_HEADER + 16 * k.stride and k.stride > 0          # ... and says what the call needs
    a.workspace_bytes = k.workspace_bytes
    assert h.dn_poisson_query(C.byref(mesh), C.byref(a), C.byref(k)) == 0


def test_the_python_predicate_is_the_querys_compact_on_every_2d_row():
    """`_auto_pack` runs before the call key and `_fused` under torch.compile: neither may make a foreign call, so they share
    ops._compact_2d; here it is held equal to what the library answers."""
    from diffnet_amd import ops
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    n = 0
    for rule in ("", "1"):
        for sizes, mkw, akw, sw, want in TABLE:
            if len(sizes) != 2 or "Q1_RULE_KERNEL" in sw or want == BADARG:
                continue
            ngp = mkw.get("ngp", 2)
            gx, gw = gauss_rule(ngp)
            geom = FemGeometry(2, sizes, tuple(1.0 / (s - 1) for s in sizes), mkw.get("deg", 1), ngp, gx, gw)
            with switches(**dict(sw, **({"Q1_RULE_KERNEL": rule} if rule else {}))):
                rc, k = query(mesh_of(sizes, **mkw), **akw)
                assert ops._compact_2d(geom, object() if akw.get("f") == "gp" else None) == (k.compact == 2), (sizes, mkw, akw, rule)
            n += 1
    assert n >= 40
