"""Every kernel variant of the stride-2 convolution families that the host dispatch can pick (csrc/conv2d_k4s2.hip, conv2d_k4s2_v2.hip,
conv3d_k4s2.hip, conv3d_wrw.hip): one table of shapes per operation, a CPU test that the tables reach every compiled instantiation
(asked of the library itself: dn_conv2d_k4s2_query / dn_conv3d_k4s2_query call the function the launch calls), and two kinds of GPU test
on every row.

EXACT.  When the weights select a single tap every output is one exact product plus exact zeros, whatever the order of the sum: the
result must be `torch.equal` to a gather of the (randn) input -- zero tolerance, no float64 reference.
    down  w[m] = 1 at (c, ky, kx) = unravel(m), M = 16 C:   coarse[b, m, i, j] = fine[b, c, 2 i + ky - 1, 2 j + kx - 1], zero in the padding
    up    w[:, c] = 1 at (m, ky, kx) = unravel(c), C = 16 M: fine[b, c, 2 i + ky - 1, 2 j + kx - 1] = coarse[b, m, i, j], zero elsewhere
    wrw   the cotangent of channel m is 1 at ONE position (b_m, i_m, j_m): gw[m, c, ky, kx] = fine[b_m, c, 2 i_m + ky - 1, 2 j_m + kx - 1];
          the probes sit on the image corners of the first and last sample and on the corners of the first and last tile of the K-slices
          (slice limits from the query)
In 3-D a channel has 64 taps; where a launch has fewer rows than selectors (M = 32 < 64 C) the selectors go through in chunks of rows.
A failure names the sample, channel, tap and position.  CPU tests show that torch's own float32 convolution gives these gathers exactly and
that a gather shifted by one row, one column or one tap does not.

BOUNDED.  With random weights, entry by entry against float64:
    |got - ref64| <= (K + 1) 2^-24 A,      A = the same contraction of |x| with |w| in float64,
K the number of products that reach one output: 16 C (down), 4 M (up), B H W (wrw).  Derivation: the matrix-core instruction is one
k-ordered chain of fp32 fused multiply-adds per output; a term of the sum passes at most K of them, whatever the order and however the
chain is cut into partial sums, so it carries at most K factors (1 + d), |d| <= u = 2^-24: |got - ref| <= gamma_K A with
gamma_K = K u / (1 - K u).  gamma_K <= (K + 1) u while K (K + 1) u <= 1, i.e. K <= 4095: the spare rounding pays for the second-order term.
The zero rows that fill a ragged K chunk add exact zeros.  The split weight gradient adds its slices in fp64 (nz 2^-53, nothing at this scale)
and rounds once to fp32, but then no term passes more than the 64 per_slice < K - 1 positions of its slice.  Where A is 0 the output must be
exactly 0 (every bounded case zeroes one channel's weights or cotangent to have such entries).  The bound only has teeth while
K^2 2^-24 << 1: these cases have C or M <= 6 and, for wrw, B H W <= 512; the deep contractions keep their max-norm tests
(tests/test_networks.py, test_gpu_round4.py).  CPU tests show a float32 evaluation inside the bound and one dropped tap far outside.

Largest |got - ref64| / bound, every bounded test prints its own (run with -s).  On the MI355X, all 135 GPU cases passing with no kernel change:
    down  v2 <32, TW, 128> 0.16-0.19   <32, TW, 64> 0.08-0.12   <64, TW, 128> and <64, TW, 64> 0.05-0.06   v1 <32> 0.08-0.10   v1 <64> 0.03-0.05
    up    v2 <32, TW, 128> 0.43-0.60   <32, TW, 64> 0.30-0.32   <64, TW, 128> and <64, TW, 64> 0.19-0.24   v1 <32> 0.24-0.47   v1 <64> 0.12-0.17
    wrw   v2 <16,64,4> 0.014 (one slice 0.049)  <32,64,4> 0.004  <64,64,4> 0.005-0.009  <16,32,8> 0.014  <32,32,8> 0.005   v1 0.005-0.10
(K = 8 or 24 for up, so single roundings show; K = 128-256 for wrw, where rounding errors grow like sqrt(K) and the bound like K.)
On the CPU a float32 evaluation of (2, 6 -> 96, 8 x 16) gives 0.046 / 0.16 / 0.010 (down / up / wrw) and one dropped tap 8.8e3 / 1.6e5 / 2.4e3 bounds.
"""
import contextlib
import ctypes as C_
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
DOWN, UP, WRW = 0, 1, 2
OPS = {DOWN: "down", UP: "up", WRW: "wrw"}


# ---------------------------------------------------------------------------------------------
# the library's own account of its dispatch
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switches(v1=False, wgs=""):
    """"CONV2D_V1" / "CONV_WRW_WGS" for the duration of one query or launch"""
    from diffnet_amd import _lib
    assert _lib.config_get("CONV2D_V1") == "" and _lib.config_get("CONV_WRW_WGS") == ""
    try:
        _lib.config_set("CONV2D_V1", "1" if v1 else "")
        _lib.config_set("CONV_WRW_WGS", wgs)
        yield
    finally:
        _lib.config_set("CONV2D_V1", "")
        _lib.config_set("CONV_WRW_WGS", "")


def query2(op, B, C, M, H, W, v1=False, wgs=""):
    from diffnet_amd import _lib
    k = _lib.DnConvK4s2Kernel()
    with switches(v1, wgs):
        rc = _lib.lib().dn_conv2d_k4s2_query(op, B, C, M, H, W, C_.byref(k))
    assert rc == 0, (rc, op, B, C, M, H, W)
    return k


def query3(op, B, C, M, D, H, W, ws=True):
    from diffnet_amd import _lib
    k = _lib.DnConvK4s2Kernel()
    rc = _lib.lib().dn_conv3d_k4s2_query(op, B, C, M, D, H, W, int(ws), C_.byref(k))
    assert rc == 0, (rc, op, B, C, M, D, H, W)
    return k


def name2(op, k):
    t = tuple(k.targ)
    if op == WRW:
        return f"wrw_v2<{t[0]},{t[1]},{t[2]}>" if k.gen == 2 else "wrw_v1"
    return f"{OPS[op]}_v2<{t[0]},{t[1]},{t[2]}>" if k.gen == 2 else f"{OPS[op]}_v1<{t[0]}>"


def wrw_extras(k):
    return {"nz=1" if k.nz == 1 else "nz>1"} | ({("", "wsum", "wsum_wave")[k.sum_kernel]} - {""})


def name3(op, k):
    if op == WRW:
        return f"wrw3d<{k.targ[0]}>"
    return f"{OPS[op]}3d<{k.targ[0]}>" + ("/split" if k.nz > 1 else "")


# ---------------------------------------------------------------------------------------------
# the tables: (B, C, M, H, W, CONV2D_V1) with the COARSE size H x W; C fine channels, M coarse channels
# ---------------------------------------------------------------------------------------------
def _rows_by_tile(small, large):
    """small / large: (contraction channels, GEMM rows) of the 32-row and the 64-row kernels"""
    rows = []
    rows += [(3, *small, H, W, False) for H, W in ((1024, 16), (512, 32), (256, 64), (128, 128), (64, 256))]      # <32, TW, 128>
    rows += [(2, *small, H, W, False) for H, W in ((8, 16), (4, 32), (2, 64), (2, 128))]                            # <32, TW, 64>
    rows += [(3, *large, H, W, False) for H, W in ((512, 16), (256, 32), (128, 64), (64, 128), (32, 256))]         # <64, TW, 128>
    rows += [(3, *large, H, W, False) for H, W in ((256, 16), (128, 32), (64, 64), (32, 128))]                      # <64, TW, 64>
    # generation 1: under the switch at a v2 shape, and of itself at widths that are no multiple of 16 (ragged last position tile)
    rows += [(2, *small, 8, 16, True), (2, *large, 4, 32, True)]
    rows += [(2, *small, 3, 5, False), (2, *small, 33, 17, False), (2, *large, 33, 17, False), (2, *large, 5, 3, False)]
    return rows


# down: rows = M = 16 C (C = 2 -> 32 rows, C = 6 -> 96 = two row tiles of 64, the second half full; 6 does not fill the second K chunk of 4)
DOWN_ROWS = _rows_by_tile((2, 32), (6, 96))
# up: rows = C = 16 M, the mirror image
UP_ROWS = [(B, C, M, H, W, v1) for B, M, C, H, W, v1 in _rows_by_tile((2, 32), (6, 96))]
# wrw: (B, C, M, H, W, CONV2D_V1)
WRW_ROWS = [
    (2, 2, 32, 4, 16, False),      # <16, 64, 4>   two slices
    (2, 6, 40, 4, 32, False),      # <32, 64, 4>   two channel groups, the second half full
    (2, 3, 70, 2, 64, False),      # <64, 64, 4>   two row groups
    (1, 2, 32, 2, 128, False),     # <64, 64, 4>   two tiles in x
    (2, 8, 32, 4, 16, False),      # <16, 32, 8>
    (2, 12, 40, 4, 32, False),     # <32, 32, 8>   two channel groups
    (1, 2, 32, 4, 16, False),      # one tile: nz = 1, written without a workspace
    (2, 2, 32, 64, 64, False),     # the U-Net's first layer in small: nz = 128, one wave per output sums the slices
    (2, 2, 32, 4, 16, True), (2, 12, 40, 4, 32, True),                      # generation 1 under the switch
    (2, 5, 33, 3, 5, False), (2, 3, 70, 33, 17, False), (2, 6, 32, 5, 3, False),   # ... and of itself
]
# 3-D: (B, C, M, D, H, W, workspace given); 105 and 45 positions per sample are no multiples of the 64-position tile
C3_DOWN_ROWS = [(2, 2, 32, 5, 3, 7, True), (2, 3, 96, 5, 3, 7, True), (2, 9, 96, 3, 5, 3, True), (2, 9, 96, 3, 5, 3, False), (1, 8, 32, 3, 5, 3, True)]
C3_UP_ROWS = [(2, 32, 2, 5, 3, 7, True), (2, 128, 4, 5, 3, 7, True), (2, 128, 16, 3, 5, 3, True), (2, 128, 16, 3, 5, 3, False), (1, 32, 16, 3, 5, 3, True)]
# 3-D wrw: (B, CN, M, d, h, w); M = 130 goes through the M > 128 block path of networks.fused._wrw3d as 128 + 2
C3_WRW_ROWS = [(1, 2, 16, 3, 4, 5), (2, 3, 20, 5, 3, 7), (2, 3, 40, 5, 3, 7), (2, 2, 130, 5, 3, 7), (2, 2, 24, 9, 8, 8)]

_TILES = [(tw, 64) for tw in (16, 32, 64)] + [(tw, 128) for tw in (16, 32, 64, 128)]
ALL_DOWN = {f"down_v2<{tm},{tw},{nt}>" for tm in (32, 64) for tw, nt in _TILES} | {"down_v1<32>", "down_v1<64>"}
ALL_UP = {f"up_v2<{tc},{tw},{nt}>" for tc in (32, 64) for tw, nt in _TILES} | {"up_v1<32>", "up_v1<64>"}
ALL_WRW = {"wrw_v2<16,64,4>", "wrw_v2<32,64,4>", "wrw_v2<64,64,4>", "wrw_v2<16,32,8>", "wrw_v2<32,32,8>", "wrw_v1", "wsum", "wsum_wave", "nz=1", "nz>1"}
ALL_3D = {"down3d<32>", "down3d<64>", "down3d<32>/split", "down3d<64>/split", "up3d<32>", "up3d<64>", "up3d<32>/split", "up3d<64>/split",
          "wrw3d<1>", "wrw3d<2>", "wrw3d<4>", "wrw3d<8>", "wsum3d_none", "wsum3d_few", "wsum3d_wave"}


def rid(row):
    return "x".join(str(int(v)) for v in row[:-1]) + ("-v1" if row[-1] is True and len(row) == 6 else "-nows" if row[-1] is False and len(row) == 7 else "")


def test_the_instantiation_lists_have_the_counts_of_the_sources():
    assert len(ALL_DOWN) == 14 + 2 and len(ALL_UP) == 14 + 2 and len(ALL_WRW) == 5 + 1 + 4


def test_tables_reach_every_compiled_variant():
    """Every instantiation of the three 2-D templates, the generation-1 kernels, both slice sums, one slice and several: asked of the
    library for every row.  A kernel that a change of the dispatch drops out of the tables is named here."""
    reached = {DOWN: set(), UP: set(), WRW: set()}
    for op, rows in ((DOWN, DOWN_ROWS), (UP, UP_ROWS), (WRW, WRW_ROWS)):
        for B, C, M, H, W, v1 in rows:
            k = query2(op, B, C, M, H, W, v1)
            reached[op].add(name2(op, k))
            if op == WRW:
                reached[op] |= wrw_extras(k)
            assert (k.gen == 1) == (v1 or W % 16 != 0), (OPS[op], B, C, M, H, W, v1, k.gen)
    for op, want in ((DOWN, ALL_DOWN), (UP, ALL_UP), (WRW, ALL_WRW)):
        assert reached[op] == want, (OPS[op], "not reached:", sorted(want - reached[op]), "unknown:", sorted(reached[op] - want))


def test_tables_hold_the_seams_the_kernels_have():
    """B > 1 (tile-to-sample decode), more than one tile in y everywhere, more than one in x wherever TW = NT (the only x seams), the
    U-Net-like wrw row (2 -> 32 channels on 64 x 64) with 128 slices summed a wave per output."""
    for op, rows in ((DOWN, DOWN_ROWS), (UP, UP_ROWS)):
        x_seams = set()
        for B, C, M, H, W, v1 in rows:
            k = query2(op, B, C, M, H, W, v1)
            assert B > 1
            if k.gen == 2:
                tm, tw, nt = k.targ
                assert H // (nt // tw) > 1, (OPS[op], H, W, tw, nt)
                assert W // tw == 1 or tw == nt, (OPS[op], H, W, tw, nt)
                if W // tw > 1:
                    x_seams.add((tm, nt))
        assert any(query2(op, *r).gen == 1 and r[3] * r[4] > 64 and (r[3] * r[4]) % 64 for r in rows)      # generation 1 with a ragged last tile
        assert x_seams == {(32, 64), (32, 128), (64, 64), (64, 128)}, (OPS[op], x_seams)
    k = query2(WRW, 2, 2, 32, 64, 64)
    assert (k.nz, k.per_slice, k.sum_kernel) == (128, 1, 2)
    assert {query2(WRW, *r[:5], r[5]).nz > 1 for r in WRW_ROWS} == {True, False}


def test_switches_act_on_the_query_as_on_the_launch():
    B, C, M, H, W = 2, 2, 32, 64, 64
    assert query2(WRW, B, C, M, H, W).gen == 2 and query2(WRW, B, C, M, H, W, v1=True).gen == 1
    assert query2(DOWN, B, C, M, H, W).gen == 2 and query2(DOWN, B, C, M, H, W, v1=True).gen == 1
    # 128 tiles: 1024 workgroups wanted -> 128 slices; 256 wanted with 8 (channel group, row group) pairs -> 32 slices of 4 tiles
    assert query2(WRW, B, 16, 256, H, W).nz == 128 and query2(WRW, B, 16, 256, H, W, wgs="256").nz == 32
    # the workspace size is the same plan
    from diffnet_amd import _lib
    for r in WRW_ROWS:
        k = query2(WRW, *r[:5], r[5])
        with switches(r[5]):
            nbytes = _lib.lib().dn_conv2d_k4s2_wrw_workspace_bytes(*r[:5])
        assert nbytes == (0 if k.nz == 1 else 4 * r[2] * r[1] * 16 * k.nz)
    k = _lib.DnConvK4s2Kernel()
    assert _lib.lib().dn_conv2d_k4s2_query(3, 1, 1, 1, 1, 1, C_.byref(k)) == -1 and _lib.lib().dn_conv2d_k4s2_query(0, 1, 1, 1, 1, 1, None) == -1
    assert _lib.lib().dn_conv2d_k4s2_query(0, 0, 1, 1, 1, 1, C_.byref(k)) == -1
    assert _lib.lib().dn_conv3d_k4s2_query(2, 1, 1, 200, 2, 2, 2, 1, C_.byref(k)) == -2          # 3-D wrw: at most 128 coarse channels per launch


def test_3d_tables_reach_both_tiles_split_and_unsplit_and_every_wrw_form():
    reached = set()
    from diffnet_amd import _lib
    for op, rows in ((DOWN, C3_DOWN_ROWS), (UP, C3_UP_ROWS)):
        for B, C, M, D, H, W, ws in rows:
            k = query3(op, B, C, M, D, H, W, ws)
            reached.add(name3(op, k))
            assert (D * H * W) % 64 != 0 and (ws or k.nz == 1)
            nbytes = _lib.lib().dn_conv3d_k4s2_workspace_bytes(op, B, C, M, D, H, W)
            kw = query3(op, B, C, M, D, H, W, True)
            assert nbytes == (0 if kw.nz == 1 else 4 * kw.nz * B * (8 * C if op == UP else M) * D * H * W)
            units = (M + 1) // 2 if op == UP else C
            assert (k.nz - 1) * k.per_slice < units <= k.nz * k.per_slice
    for B, CN, M, d, h, w in C3_WRW_ROWS:
        for m0 in range(0, M, 128):
            k = query3(WRW, B, CN, min(128, M - m0), d, h, w)
            reached |= {name3(WRW, k), ("wsum3d_none", "wsum3d_few", "wsum3d_wave")[k.sum_kernel]}
    assert reached == ALL_3D, ("not reached:", sorted(ALL_3D - reached), "unknown:", sorted(reached - ALL_3D))


# ---------------------------------------------------------------------------------------------
# single-tap weights and the gathers they must give (any number of space dimensions)
# ---------------------------------------------------------------------------------------------
def selectors(channels, nd):
    """(channel, tap) in the row-major order of unravel(index)"""
    return [(c, tap) for c in range(channels) for tap in itertools.product(range(4), repeat=nd)]


def tap_view(tap, size):
    """padded fine coordinates 2 i + k of tap k over the coarse grid: the strided window of F.pad(fine, 1)"""
    return tuple(slice(k, k + 2 * n, 2) for k, n in zip(tap, size))


def down_weights(sel, C, nd):
    w = torch.zeros((len(sel), C) + (4,) * nd)
    for m, (c, tap) in enumerate(sel):
        w[(m, c) + tap] = 1.0
    return w


def down_gather(fine, sel, size, shift=(0, 0)):
    """coarse[b, m] = fine[b, c, 2 i + k - 1] with zero padding; shift = (rows, columns) moves the gather (the CPU tests' wrong answers)"""
    nd = len(size)
    fp = F.pad(fine, (1, 1) * nd)
    if any(shift):
        fp = torch.roll(fp, shift, (-2, -1))
    return torch.stack([fp[(slice(None), c) + tap_view(tap, size)] for c, tap in sel], 1)


def up_weights(sel, M, nd):
    w = torch.zeros((M, len(sel)) + (4,) * nd)
    for c, (m, tap) in enumerate(sel):
        w[(m, c) + tap] = 1.0
    return w


def up_scatter(coarse, sel, size, shift=(0, 0)):
    """fine[b, c, 2 i + k - 1] = coarse[b, m, i], zero at the other parities"""
    nd = len(size)
    ep = torch.zeros((coarse.shape[0], len(sel)) + tuple(2 * n + 2 for n in size))
    for c, (m, tap) in enumerate(sel):
        ep[(slice(None), c) + tap_view(tap, size)] = coarse[:, m]
    if any(shift):
        ep = torch.roll(ep, shift, (-2, -1))
    return ep[(Ellipsis,) + (slice(1, -1),) * nd].contiguous()


def wrw_probes(B, M, size, k, gen2_tile=None):
    """One (sample, position) per coarse channel: the corners of the first and the last sample, then the corners of the first and last tile
    of the K-slices of the launch `k` describes.  gen2_tile = (TW, NT) for the raw-row-tile kernels, whose tiles are TR x TW blocks."""
    nd = len(size)
    corners = [(b,) + tuple(p) for b in sorted({0, B - 1}) for p in itertools.product(*[sorted({0, n - 1}) for n in size])]
    npos = 1
    for n in size:
        npos *= n
    seams = []
    if gen2_tile is None:
        def unravel(p):
            out = []
            for n in reversed(size):
                out.append(p % n)
                p //= n
            return (p,) + tuple(reversed(out))
        for z in range(k.nz):
            first, last = 64 * k.per_slice * z, min(64 * k.per_slice * (z + 1), B * npos) - 1
            seams += [unravel(first), unravel(min(first + 63, last)), unravel(last - (last - first) % 64), unravel(last)]
    else:
        tw, nt = gen2_tile
        tr, (H, W) = nt // tw, size
        tiles_x, per = W // tw, (64 // nt) * k.per_slice
        nblocks = B * (H // tr) * tiles_x
        for z in range(k.nz):
            for t in sorted({per * z, min(per * (z + 1), nblocks) - 1}):
                b, ts = divmod(t, (H // tr) * tiles_x)
                i0, j0 = (ts // tiles_x) * tr, (ts % tiles_x) * tw
                seams += [(b, i0, j0), (b, i0, j0 + tw - 1), (b, i0 + tr - 1, j0), (b, i0 + tr - 1, j0 + tw - 1)]
    room = max(M - len(corners), 0)
    if len(seams) > room:                                   # evenly spread, first and last kept
        seams = [seams[(q * (len(seams) - 1)) // max(room - 1, 1)] for q in range(room)]
    cands = corners + seams
    return [cands[m % len(cands)] for m in range(M)]


def wrw_cotangent(probes, B, size):
    cot = torch.zeros((B, len(probes)) + tuple(size))
    for m, p in enumerate(probes):
        cot[(p[0], m) + tuple(p[1:])] = 1.0
    return cot


def wrw_gather(fine, probes, nd, shift=0):
    """gw[m, c, taps] = fine[b_m, c, 2 i_m + k - 1]: the 4^nd window of the padded input at twice the probe position"""
    fp = F.pad(fine, (1, 1 + shift) * nd)
    return torch.stack([fp[(p[0], slice(None)) + tuple(slice(2 * i + shift, 2 * i + shift + 4) for i in p[1:])] for p in probes], 0)


def mismatch(got, want):
    """'' when equal, else the index of the first entry that differs with both values"""
    if got.shape == want.shape and torch.equal(got, want):
        return ""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = (got != want).nonzero()
    idx = tuple(int(v) for v in bad[0])
    return f"{len(bad)} entries differ, first at {idx}: got {float(got[idx])!r}, want {float(want[idx])!r}"


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------
# CPU: the gathers are what a convolution with these weights gives, and a shifted gather is not
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [2, 3])
def test_single_tap_weights_make_torch_reproduce_the_gather_exactly(nd):
    size = (8, 16) if nd == 2 else (3, 2, 5)
    conv, convt = (F.conv2d, F.conv_transpose2d) if nd == 2 else (F.conv3d, F.conv_transpose3d)
    B, C = 2, 6 if nd == 2 else 2
    sel = selectors(C, nd)
    fine = randn((B, C) + tuple(2 * n for n in size), 1)
    w = down_weights(sel, C, nd)
    got = conv(fine, w, None, 2, 1)
    assert mismatch(got, down_gather(fine, sel, size)) == ""
    assert not torch.equal(got, down_gather(fine, sel, size, (1, 0))) and not torch.equal(got, down_gather(fine, sel, size, (0, 1)))
    assert not torch.equal(got, down_gather(fine, sel[1:] + sel[:1], size))                               # one tap further
    # up: ConvTranspose with (cin = M, cout = C) weights
    M = C
    coarse = randn((B, M) + size, 2)
    wu = up_weights(sel, M, nd)
    gotu = convt(coarse, wu, None, 2, 1)
    assert mismatch(gotu, up_scatter(coarse, sel, size)) == ""
    assert not torch.equal(gotu, up_scatter(coarse, sel, size, (1, 0))) and not torch.equal(gotu, up_scatter(coarse, sel, size, (0, 1)))
    assert not torch.equal(gotu, up_scatter(coarse, sel[1:] + sel[:1], size))
    # wrw: the weight gradient of the convolution for a cotangent with one 1 per channel
    Mw = 40
    k = query2(WRW, B, C, Mw, *size) if nd == 2 else query3(WRW, B, C, Mw, *size)
    tile = (k.targ[0], k.targ[1]) if nd == 2 and k.gen == 2 else None
    probes = wrw_probes(B, Mw, size, k, tile)
    assert len(set(probes)) >= 2 ** nd + 1 and all(0 <= p[0] < B and all(0 <= i < n for i, n in zip(p[1:], size)) for p in probes)
    ww = torch.zeros((Mw, C) + (4,) * nd, requires_grad=True)
    gw, = torch.autograd.grad(conv(fine, ww, None, 2, 1), ww, wrw_cotangent(probes, B, size))
    assert mismatch(gw, wrw_gather(fine, probes, nd)) == ""
    assert not torch.equal(gw, wrw_gather(fine, probes, nd, 1))


# ---------------------------------------------------------------------------------------------
# float64 references and the bound
# ---------------------------------------------------------------------------------------------
def ref_down(fine, w):
    """(B, M, H, W) in the dtype of the arguments, by unfolding: patches (B, 16 C, H W)"""
    B, C, H2, W2 = fine.shape
    p = F.unfold(fine, 4, padding=1, stride=2)
    return torch.einsum("mk,bkp->bmp", w.reshape(w.shape[0], -1), p).reshape(B, w.shape[0], H2 // 2, W2 // 2)


def ref_up(coarse, w):
    return F.conv_transpose2d(coarse, w, None, 2, 1)


def ref_wrw(fine, coarse):
    B, M = coarse.shape[:2]
    p = F.unfold(fine, 4, padding=1, stride=2)
    return torch.einsum("bmp,bkp->mk", coarse.reshape(B, M, -1), p).reshape(M, fine.shape[1], 4, 4)


def ratio_to_bound(got, ref, A, K, what):
    """largest |got - ref| / ((K + 1) 2^-24 A); where A is 0, got must be exactly 0"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    zero = A == 0
    assert bool((got[zero] == 0).all()), (what, "entries with no term are not exactly zero")
    r = ((got - ref).abs()[~zero] / ((K + 1) * U24 * A[~zero])).max()
    return float(r)


@functools.lru_cache(maxsize=4)
def bounded_case(op, B, C, M, H, W):
    """inputs (fp32), float64 reference and absolute-value contraction of one bounded case, with one all-zero channel"""
    fine, coarse, w = randn((B, C, 2 * H, 2 * W), 5), randn((B, M, H, W), 6), randn((M, C, 4, 4), 7)
    if op == DOWN:
        w[1] = 0
        return (fine, w), ref_down(fine.double(), w.double()), ref_down(fine.double().abs(), w.double().abs()), 16 * C
    if op == UP:
        w[:, 1] = 0
        return (coarse, w), ref_up(coarse.double(), w.double()), ref_up(coarse.double().abs(), w.double().abs()), 4 * M
    coarse[:, 1] = 0
    return (fine, coarse), ref_wrw(fine.double(), coarse.double()), ref_wrw(fine.double().abs(), coarse.double().abs()), B * H * W


@pytest.mark.parametrize("op,B,C,M,H,W", [(DOWN, 2, 6, 96, 8, 16), (UP, 2, 96, 6, 8, 16), (WRW, 2, 6, 40, 8, 16)])
def test_float32_evaluation_is_inside_the_bound_and_a_dropped_tap_far_outside(op, B, C, M, H, W):
    args, ref, A, K = bounded_case(op, B, C, M, H, W)
    fn = (ref_down, ref_up, ref_wrw)[op]
    r = ratio_to_bound(fn(*args), ref, A, K, OPS[op])
    print(f"float32 on the CPU, {OPS[op]} ({B}, {C}, {M}, {H}x{W}): |err| / bound {r:.3f}")
    assert r <= 1.0
    a0, a1 = args[0].clone(), args[1].clone()
    if op == WRW:
        a0[1, 3, 5, 7] = 0          # the tap of one position
    else:
        a1[5, 3, 2, 1] = 0          # one tap of one channel pair
    bad = fn(a0, a1).double()
    zero = A == 0
    rb = float(((bad - ref).abs()[~zero] / ((K + 1) * U24 * A[~zero])).max())
    print(f"   one dropped tap: {rb:.3g} bounds")
    assert rb > 100.0


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda", 0)


def launch2(op, a, b, v1):
    """one launch through the thin wrappers of networks.fused (contiguous fp32 device tensors, 16-byte aligned)"""
    from diffnet_amd.networks import fused
    a, b = a.to(dev()), b.to(dev())
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    with switches(v1):
        out = (fused._c2_down, fused._c2_up, fused._c2_wrw)[op](a, b)
        torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("row", DOWN_ROWS, ids=rid)
def test_down_single_tap_is_an_exact_gather(row):
    B, C, M, H, W, v1 = row
    sel = selectors(C, 2)
    assert len(sel) == M
    fine = randn((B, C, 2 * H, 2 * W), 21)
    got = launch2(DOWN, fine, down_weights(sel, C, 2), v1)
    what = mismatch(got, down_gather(fine, sel, (H, W)))
    assert what == "", (name2(DOWN, query2(DOWN, B, C, M, H, W, v1)), "index (b, m = 16 c + 4 ky + kx, i, j):", what)


@pytest.mark.gpu
@pytest.mark.parametrize("row", UP_ROWS, ids=rid)
def test_up_single_tap_is_an_exact_scatter(row):
    B, C, M, H, W, v1 = row
    sel = selectors(M, 2)
    assert len(sel) == C
    coarse = randn((B, M, H, W), 22)
    got = launch2(UP, coarse, up_weights(sel, M, 2), v1)
    what = mismatch(got, up_scatter(coarse, sel, (H, W)))
    assert what == "", (name2(UP, query2(UP, B, C, M, H, W, v1)), "index (b, c = 16 m + 4 ky + kx, y, x):", what)


@pytest.mark.gpu
@pytest.mark.parametrize("row", WRW_ROWS, ids=rid)
def test_wrw_single_position_cotangent_is_an_exact_gather(row):
    B, C, M, H, W, v1 = row
    k = query2(WRW, B, C, M, H, W, v1)
    probes = wrw_probes(B, M, (H, W), k, (k.targ[0], k.targ[1]) if k.gen == 2 else None)
    fine = randn((B, C, 2 * H, 2 * W), 23)
    got = launch2(WRW, fine, wrw_cotangent(probes, B, (H, W)), v1)
    what = mismatch(got, wrw_gather(fine, probes, 2))
    bad = "" if what == "" else f"{what}; probe of that channel (b, i, j): {probes[int(what.split('(')[1].split(',')[0])]}"
    assert what == "", (name2(WRW, k), f"nz {k.nz} per_slice {k.per_slice}", "index (m, c, ky, kx):", bad)


def _bounded(op, row):
    B, C, M, H, W, v1 = row
    args, ref, A, K = bounded_case(op, B, C, M, H, W)
    got = launch2(op, *args, v1)
    k = query2(op, B, C, M, H, W, v1)
    r = ratio_to_bound(got, ref, A, K, name2(op, k))
    print(f"{name2(op, k)} ({B}, {C}, {M}, {H}x{W}) K = {K}: |err| / bound {r:.3f}")
    assert r <= 1.0, (name2(op, k), r)


@pytest.mark.gpu
@pytest.mark.parametrize("row", DOWN_ROWS, ids=rid)
def test_down_within_the_summation_bound(row):
    _bounded(DOWN, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", UP_ROWS, ids=rid)
def test_up_within_the_summation_bound(row):
    _bounded(UP, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in WRW_ROWS if r[0] * r[3] * r[4] <= 512], ids=rid)
def test_wrw_within_the_summation_bound(row):
    _bounded(WRW, row)


# ---- 3-D ------------------------------------------------------------------------------------
def launch3(op, src, w, B, C, M, D, H, W, ws):
    """dn_conv3d_k4s2_down_ws / _up_ws with the workspace the library asks for, or the unsplit launch"""
    from diffnet_amd import _lib
    L = _lib.lib()
    src, w = src.to(dev()).contiguous(), w.to(dev()).contiguous()
    out = torch.empty((B, C, 2 * D, 2 * H, 2 * W) if op == UP else (B, M, D, H, W), device=dev())
    nbytes = L.dn_conv3d_k4s2_workspace_bytes(op, B, C, M, D, H, W) if ws else 0
    assert nbytes >= 0
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())
    s = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C_.c_void_p(t.data_ptr())
    fn = L.dn_conv3d_k4s2_up_ws if op == UP else L.dn_conv3d_k4s2_down_ws
    rc = fn(p(src), p(w), p(out), B, C, M, D, H, W, p(work) if ws else None, nbytes, s)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("row", C3_DOWN_ROWS, ids=rid)
def test_down3d_single_tap_is_an_exact_gather(row):
    B, C, M, D, H, W, ws = row
    sel = selectors(C, 3)
    assert len(sel) % M == 0
    fine = randn((B, C, 2 * D, 2 * H, 2 * W), 31)
    for s0 in range(0, len(sel), M):                     # 64 C selectors, M of them per launch
        part = sel[s0:s0 + M]
        got = launch3(DOWN, fine, down_weights(part, C, 3), B, C, M, D, H, W, ws)
        what = mismatch(got, down_gather(fine, part, (D, H, W)))
        assert what == "", (name3(DOWN, query3(DOWN, B, C, M, D, H, W, ws)), f"selectors {s0}.., index (b, m, i, j, k):", what)


@pytest.mark.gpu
@pytest.mark.parametrize("row", C3_UP_ROWS, ids=rid)
def test_up3d_single_tap_is_an_exact_scatter(row):
    B, C, M, D, H, W, ws = row
    sel = selectors(M, 3)
    assert len(sel) % C == 0
    coarse = randn((B, M, D, H, W), 32)
    for s0 in range(0, len(sel), C):
        part = sel[s0:s0 + C]
        got = launch3(UP, coarse, up_weights(part, M, 3), B, C, M, D, H, W, ws)
        what = mismatch(got, up_scatter(coarse, part, (D, H, W)))
        assert what == "", (name3(UP, query3(UP, B, C, M, D, H, W, ws)), f"selectors {s0}.., index (b, c, z, y, x):", what)


@pytest.mark.gpu
@pytest.mark.parametrize("row", C3_WRW_ROWS, ids=lambda r: "x".join(map(str, r)))
def test_wrw3d_single_position_cotangent_is_an_exact_gather(row):
    from diffnet_amd.networks import fused
    B, CN, M, d, h, w = row
    probes = []
    for m0 in range(0, M, 128):                          # the probes of each block of 128 channels follow that launch's own slices
        mb = min(128, M - m0)
        probes += wrw_probes(B, mb, (d, h, w), query3(WRW, B, CN, mb, d, h, w))
    fine = randn((B, CN, 2 * d, 2 * h, 2 * w), 33)
    got = fused._wrw3d(fine.to(dev()), wrw_cotangent(probes, B, (d, h, w)).to(dev())).cpu()
    what = mismatch(got, wrw_gather(fine, probes, 3))
    assert what == "", ("index (m, cn, kz, ky, kx):", what)
