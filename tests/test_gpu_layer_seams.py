"""The network-layer kernels -- InstanceNorm + activation (csrc/instnorm_act.hip), the fused Upsample -> Conv -> Sigmoid output blocks
(upconv_out.hip, upconv3d_out.hip), the stride-1 valid convolutions (conv2d_direct.hip) -- against float64 at every dispatch seam: the
slice counts of the sliced InstanceNorm (2, 8, the cap 64, 63 limited by the instance count, the n_inst >= 2048 return), its block-size and
float4 seams, views whose storage is one float off, the multi-tile loop of both weight-gradient kernels (tiles_per_wg 2, an empty trailing
tile, tiles that straddle samples), the vec16 staging with C < 64, C > 64 and a misaligned input, missing biases, K = 1 and 1 x 1 outputs.
CPU tests ask the library's own size functions which branch each row of the tables takes, and show that every bound rejects a wrong operator.

The comparison is a derived bound, as in test_gpu_dropin_seams.py: reference and magnitude field A in float64 from the same float32 inputs,
    |got - ref| <= n 2^-24 A   entry by entry,  and exactly 0 where A is 0,
n the number of roundings a term can pass (gamma_n holds for any order of the sum).  u = 2^-24 below.

INSTANCE NORM, forward.  mu, r = 1 / sqrt(var + eps) in float64 (two passes), t = (x - mu) r, ref = act(t), L = max(1, |slope|).  The kernel
has m = fl(mu') and fl(r') with mu', r' its own fp64 statistics (relative error << 2^-40, see below), and computes fl(fl(fl(x - m) fl(r)) slope):
    x - m = (x - mu) + (mu - m):  |mu - m| <= u |mu|  moves t by |mu| r u;  the subtraction, fl(r) and the product: 3 u |t|;
    the activation is L-Lipschitz (no mask around the kink): both move y by at most L times that;  the slope product adds u |y|:
    |y - ref| <= u (L (3 |t| + |mu| r) + |ref|) (1 + 1e-3).
The saved statistics: |mean - mu| <= (u + 2^-40) |mu|, |rstd - r| <= (u + 2^-40) r.  This is the check that found the one kernel bug of this
suite: the sums were of x and x^2, so var = E[x^2] - mu^2 cancelled when |mu| >> spread -- with mean 1000 and spread 0.01 rstd was off by
15 .. 350 u (S = 1e3 .. 5e5, float64 emulation of the kernel's order; on the MI355X 1.6 .. 68 u in 19 of the 23 InstanceNorm cases here),
unnoticed by a max-norm 2e-5.  The kernel now sums x - x[0] (test_instnorm_rstd_bound_rejects_unshifted_sums restates both forms).
INSTANCE NORM, backward, with the saved float32 mean and rstd as data of the reference (so sign(h) is the kernel's and act' is selected
identically): gx = r (g - mean g - h mean(g h)), A = r (|g| + mean|g| + |h| mean|g h|).  Roundings: h = fl(fl(x - m) r) 2, g = fl(gy slope) 1,
mean g = fl(fp64 sum / S) 1 + 1, mean(g h) = fl(fp64 sum of exact products) 1 + 1 + 2, then g - mg, the fma with h mgx, the product with r: 3.
Worst term h mean(g h): 2 + 4 + 2 = 8, + 1 for the second order: n = 9.

OUTPUT BLOCKS.  EXACT: act = 0, no bias, weight 1 at one (c0, tap): forward and input gradient are gathers (layers_ref.upconv_gather*) and
must be torch.equal.  BOUNDED, A = the same composition of |x|, |w|, |b| (and |gout| y (1 - y) for a given y in (0, 1): gz = fl(fl(gout y) fl(1 - y)), 3):
    forward 2-D   C + 14: effective-weight presums 3, the per-channel expression <= 9, one add per channel C, bias start 1, + 1
    forward 3-D   8 C + 9: presums of <= 8 taps 7, one fma chain of 8 per channel carried through the channels 8 C, bias start 1, + 1
    input grad    2-D 32 = presums 3 + gz 3 + a chain of 25 fmas + 1;   3-D 75 = 7 + 3 + 64 + 1
    weight grad   128 tiles_per_wg + 8: gz 3, box sums 3 (2-D: two levels and the bias pick; 3-D: three pair sums), the fp32 matrix-core
                  instruction as one k-ordered fma chain (the model of test_gpu_conv_variants.py) over 128 pixels per tile, carried over
                  the workgroup's tiles; the fp64 sum over workgroups is rounded once; + 1
    bias grad     2-D tiles_per_wg + 8: gz 3, box 2, one add per tile, fl(block sum) 1, fl(sum over workgroups) 1, + 1;  3-D one more box level: + 9
SIGMOID: y(act = 1) against the float64 sigmoid of the SAME inputs' act = 0 output z (bitwise the same z: act is a runtime flag after the sum),
    e = |y - s64(z)| / (u s (1 + (1 - s)(1 + |z|))),   z spanning +-20.
The accuracy of __expf is not derivable from the source; e is measured and capped at twice the measurement, rounded up (see SIGMOID_CAP).

VALID CONVOLUTION: forward Ci K^2 + 1 (one fma chain from the bias), input gradient Co K^2 (a chain from 0; + 0: the first fma is exact),
weight and bias gradients 2 (fp64 products and sums, rounded once).

Largest |got - ref| / bound per family on the MI355X (every test prints its own; run with -s):
    InstanceNorm forward      y 0.67     mean 0.68     rstd 0.85   (rstd: rounding the fp64 value to float32 is already half the bound)
    InstanceNorm backward     0.25       views one float off: the same figures as their aligned runs (y 0.50, rstd 0.80, gx 0.19)
    output block 2-D          forward 0.13    input gradient 0.12    weight gradient 0.012    bias gradient 0.11
    output block 3-D          forward 0.10    input gradient 0.042   weight gradient 0.012    bias gradient 0.034
    ... at tiles_per_wg = 2   weight gradient 4e-5 .. 7e-5, bias gradient 1e-5 .. 1.2e-4 (393 344 .. 532 480 terms: errors grow like the root of that)
    sigmoid                   e = 1.48 (2-D), 1.46 (3-D)  ->  SIGMOID_CAP = 3
    valid convolution         forward 0.43    input gradient 0.28    weight gradient 0.47     bias gradient 0.05
All 61 GPU cases pass with the shifted InstanceNorm sums; no other kernel needed a change.  On the CPU a float32 evaluation gives
InstanceNorm 0.82 (mean at S = 2) / 0.8 / 0.22, output blocks 0.19 / 0.047 / 0.0099 / 0.028, and the wrong operators 1e2 .. 5e6 bounds.
"""
import functools
import itertools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import layers_ref as R
from test_gpu_dropin_seams import bound_ratio, U
from test_gpu_parity import dev

EPS = 1e-5
EPS64 = float(torch.tensor(EPS, dtype=torch.float32))       # what reaches the kernel through its float argument
STAT_N = 1.0 + 2.0 ** -40 / U                                # (u + 2^-40) in units of u
SIGMOID_CAP = 3                                              # twice the largest e measured on the MI355X (1.48), rounded up
RATIOS = {}


def check(family, case, **parts):
    """parts: name -> (got, ref, A, n).  Prints every ratio, then asserts each is within the bound."""
    rs = {k: bound_ratio(*v) for k, v in parts.items()}
    RATIOS[family] = max(RATIOS.get(family, 0.0), *rs.values())
    print(f"layer-ratio {family} {case}: " + " ".join(f"{k}={r:.3g}" for k, r in rs.items()) + f" (family max so far {RATIOS[family]:.3g})")
    for k, r in rs.items():
        assert r <= 1.0, f"{family} {case} {k}: |got - ref| is {r:.3g} x the bound"
    return rs


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def randn(shape, *key):
    return torch.randn(shape, generator=gen(*key))


def rand(shape, *key):
    return torch.rand(shape, generator=gen(*key))


def lib():
    from diffnet_amd import _lib
    return _lib.lib()


def ptr(t):
    from diffnet_amd.ops import _p
    return _p(t)


def stream(t):
    from diffnet_amd.ops import _stream
    return _stream(t)


def one_float_off(t):
    """a contiguous view with t's values whose storage starts one float into a fresh allocation"""
    v = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1
    return v


def workspace(nbytes, device):
    assert nbytes >= 0, nbytes
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


# ---------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------
# InstanceNorm: shape, kind of the first instance, expected (nchunk, threads of the one-pass kernel or None, float4), slopes
ALL_SLOPES = (0.2, 0.0, 1.0)
IN_ROWS = [
    ((2, 3, 1, 2), 0, (1, 64, False), ALL_SLOPES),
    ((2, 3, 7, 9), 1, (1, 64, False), ALL_SLOPES),                 # S = 63
    ((1, 5, 8, 8), 2, (1, 64, True), ALL_SLOPES),                  # 64
    ((2, 2, 5, 13), 3, (1, 64, False), ALL_SLOPES),                # 65
    ((1, 3, 3, 11, 31), 0, (1, 64, False), ALL_SLOPES),            # 1023
    ((2, 3, 32, 32), 1, (1, 64, True), ALL_SLOPES),                # 1024: the last size of the 64-thread kernel
    ((1, 3, 25, 41), 2, (1, 256, False), ALL_SLOPES),              # 1025
    ((2, 2, 4, 257), 3, (1, 256, True), ALL_SLOPES),               # 1028
    ((1, 2, 4, 63, 65), 1, (1, 256, True), ALL_SLOPES),            # 16380: the last float4 size below the sliced path
    ((1, 3, 127, 129), 0, (1, 256, False), ALL_SLOPES),            # 16383
    ((32, 64, 128, 128), 0, (1, 256, True), (0.2,)),               # n_inst = 2048 at a sliced size
    ((1, 2, 128, 128), 1, (2, None, True), ALL_SLOPES),            # (2, 16384)
    ((1, 3, 5, 3277), 0, (2, None, False), ALL_SLOPES),            # (3, 16385): ragged last slice
    ((1, 1, 4, 16385), 2, (8, None, True), ALL_SLOPES),            # (1, 65540): last slice shorter
    ((1, 1, 64, 64, 128), 1, (64, None, True), ALL_SLOPES),        # (1, 524288): the cap
    ((3, 11, 64, 64, 128), 0, (63, None, True), ALL_SLOPES),       # (33, 524288): limited by n_inst, slices of 8324
]
IN_IDS = ["x".join(map(str, r[0])) for r in IN_ROWS]


def in_sizes(shape):
    return shape[0] * shape[1], math.prod(shape[2:])


def in_nchunk(n_inst, S):
    """the planner's slice count, from dn_instnorm_workspace_bytes = 16 n_inst nchunk (0: one pass)"""
    nbytes = lib().dn_instnorm_workspace_bytes(n_inst, S)
    assert nbytes >= 0 and nbytes % (16 * n_inst) == 0, nbytes
    return nbytes // (16 * n_inst) or 1


# output blocks, backward: (B, C, h, w) or (B, C, d, h, w), input one float off, expected (tiles_per_wg, vec16, channel passes,
# empty trailing tile, tiles straddle samples)
UC2_ROWS = [
    ((1, 3, 3073, 128), False, (2, True, 1, True, False)),
    ((3, 2, 363, 363), False, (2, False, 1, True, True)),
    ((1, 2, 628, 627), False, (2, False, 1, True, False)),
    ((2, 70, 16, 16), False, (1, True, 2, False, False)),
    ((2, 5, 16, 8), False, (1, True, 1, False, False)),
    ((2, 64, 16, 16), True, (1, False, 1, False, False)),
    ((1, 65, 7, 9), False, (1, False, 2, False, False)),
]
UC3_ROWS = [
    ((1, 2, 81, 81, 81), False, (2, False, 1, False, False)),
    ((2, 2, 64, 65, 64), False, (2, False, 1, False, False)),
    ((1, 33, 3, 4, 66), False, (1, False, 2, False, False)),
    ((2, 31, 2, 2, 2), False, (1, False, 1, False, False)),
]
UC_IDS = lambda rows: ["x".join(map(str, r[0])) + ("_off1" if r[1] else "") for r in rows]      # noqa: E731
UC_TILE = 128
UC_CCH = {2: 64, 3: 32}


def uc_plan(shape):
    """(nwg, tiles, tiles_per_wg) from the workspace size: 4 (50 C + nwg (16 C + 1)) in 2-D, 4 (128 C + nwg (27 C + 1)) in 3-D"""
    nd, C = len(shape) - 2, shape[1]
    nbytes = (lib().dn_upconv_out_workspace_bytes if nd == 2 else lib().dn_upconv3d_out_workspace_bytes)(shape[0], C, *shape[2:])
    fixed, per = (50 * C, 16 * C + 1) if nd == 2 else (128 * C, 27 * C + 1)
    nwg, rem = divmod(nbytes // 4 - fixed, per)
    assert nbytes > 0 and nbytes % 4 == 0 and rem == 0 and nwg >= 1, (shape, nbytes)
    tiles = -(-shape[0] * math.prod(shape[2:]) // UC_TILE)
    return nwg, tiles, -(-tiles // nwg)


CV_ROWS = [(1, 1, 1, 7, 7, 7, True), (2, 3, 5, 4, 6, 1, True), (3, 3, 5, 9, 11, 5, True), (3, 3, 5, 9, 11, 5, False), (1, 2, 3, 20, 19, 3, True)]
CV_IDS = ["x".join(map(str, r[:6])) + ("" if r[6] else "_nobias") for r in CV_ROWS]


# ---------------------------------------------------------------------------------------------
# 1. CPU: the tables reach every branch (asked of the library's size functions, not restated)
# ---------------------------------------------------------------------------------------------
def test_instnorm_table_reaches_every_branch():
    seen = set()
    for shape, _, (nchunk, block, vec), _ in IN_ROWS:
        n_inst, S = in_sizes(shape)
        assert in_nchunk(n_inst, S) == nchunk, (shape, in_nchunk(n_inst, S))
        assert (S % 4 == 0) == vec, shape                              # Slice::vec on 16-byte aligned tensors
        if nchunk == 1:
            assert block == (64 if S <= 1024 else 256), shape         # the host's S <= 1024 seam
            seen.add(("one pass", block, vec))
        else:
            length = (-(-S // nchunk) + 3) & ~3                        # slice_of's slice length
            seen.add(("sliced", nchunk, vec, "ragged" if S % length else "even"))
    assert seen >= {("one pass", b, v) for b in (64, 256) for v in (False, True)}
    assert {s[1] for s in seen if s[0] == "sliced"} == {2, 8, 63, 64}
    # both sides of the seams: 1024 | 1025, 16380 | 16384 at n_inst 2, 2047 | 2048 instances at S = 16384, the cap and the count below it
    assert in_nchunk(2, 16383) == 1 and in_nchunk(2, 16384) == 2
    assert in_nchunk(2047, 16384) == 2 and in_nchunk(2048, 16384) == 1
    assert in_nchunk(1, 524288) == 64 and in_nchunk(1, 1 << 22) == 64 and in_nchunk(33, 524288) == 63
    assert (-(-524288 // 63) + 3) & ~3 == 8324
    assert in_nchunk(4, 65540) == 8                                    # the channel-slice case
    # a view one float off is never float4: its byte offset is 4 mod 16 whatever the allocation's alignment (>= 16 bytes, asserted on the GPU)
    v = one_float_off(torch.zeros(2, 3, 32, 32))
    assert (v.data_ptr() - v.untyped_storage().data_ptr()) % 16 == 4


@pytest.mark.parametrize("rows", [UC2_ROWS, UC3_ROWS], ids=["2d", "3d"])
def test_output_block_tables_reach_every_branch(rows):
    seen = set()
    for shape, off, (tpw, vec16, passes, trailing, straddle) in rows:
        nd, (B, C) = len(shape) - 2, shape[:2]
        nwg, tiles, got_tpw = uc_plan(shape)
        plane = math.prod(shape[2:])
        assert got_tpw == tpw, (shape, nwg, tiles, got_tpw)
        assert (nwg * tpw > tiles) == trailing, (shape, nwg, tiles)
        assert -(-C // UC_CCH[nd]) == passes, shape
        assert (B > 1 and plane % UC_TILE != 0 and tpw > 1) == straddle, shape
        if nd == 2:
            assert (plane % UC_TILE == 0 and not off) == vec16, shape             # the host's vec16 condition; `off` puts `in` at 4 mod 16
            seen.add((tpw, vec16, passes))
        else:
            seen.add((tpw, passes, C % UC_CCH[nd] != 0))
    if rows is UC2_ROWS:
        assert seen >= {(2, True, 1), (2, False, 1), (1, True, 2), (1, True, 1), (1, False, 1), (1, False, 2)}
        assert uc_plan((1, 3, 3072, 128))[2] == 1 and uc_plan((1, 64, 512, 512))[2] == 1      # the other side; the largest shape of the older tests
    else:
        assert seen >= {(2, 1, True), (1, 2, True), (1, 1, True)}
        assert uc_plan((1, 2, 64, 64, 128))[2] == 1 and uc_plan((1, 2, 16, 16, 16))[2] == 1


# ---------------------------------------------------------------------------------------------
# 2. InstanceNorm + activation
# ---------------------------------------------------------------------------------------------
KIND_MEAN = torch.tensor([1.5, 1000.0, -7.0, 2.75])          # benign, large mean, tiny spread, constant
KIND_STD = torch.tensor([3.0, 0.01, 1e-3, 0.0])


def in_data(n_inst, S, first, *key):
    k = (first + torch.arange(n_inst)) % 4
    return KIND_MEAN[k][:, None] + KIND_STD[k][:, None] * randn((n_inst, S), "in x", n_inst, S, first, *key)


@functools.lru_cache(maxsize=1)
def in_problem(n_inst, S, first):
    """float32 x and cotangent, and, computed once and left unchanged, x in float64 with its float64 statistics"""
    x = in_data(n_inst, S, first)
    gy = randn((n_inst, S), "in gy", n_inst, S, first)
    x64 = x.double()
    mu, r = R.instnorm_stats(x64, EPS64)
    return x, gy, x64, mu, r


def in_fwd_bound(x64, mu, r, slope):
    """(ref, A, n) of the forward bound"""
    ref, t = R.instnorm_fwd(x64, mu, r, slope)
    return ref, (max(1.0, abs(slope)) * (3 * t.abs() + mu.abs() * r) + ref.abs()) * (1 + 1e-3), 1


def in_fwd_parts(y, mean, rstd, x64, mu, r, slope):
    ref, A, n = in_fwd_bound(x64, mu, r, slope)
    parts = dict(y=(y.reshape(ref.shape), ref, A, n))
    if mean is not None:
        parts.update(mean=(mean.reshape(mu.shape), mu, mu.abs(), STAT_N), rstd=(rstd.reshape(r.shape), r, r, STAT_N))
    return parts


def in_bwd_parts(gx, x64, gy, mean, rstd, slope):
    ref, A = R.instnorm_bwd(x64, gy.double(), mean.double().cpu().reshape(-1, 1), rstd.double().cpu().reshape(-1, 1), slope)
    return dict(gx=(gx.reshape(ref.shape), ref, A, 9))


def in_fwd_c(x, slope):
    """x (n_inst, S) on the GPU -> y, mean, rstd through the C ABI"""
    n_inst, S = x.shape
    y, mean = torch.empty(x.shape, dtype=torch.float32, device=x.device), torch.empty(n_inst, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    assert y.data_ptr() % 16 == 0                                      # outputs are never misaligned
    nbytes = lib().dn_instnorm_workspace_bytes(n_inst, S)
    ws = workspace(nbytes, x.device)
    rc = lib().dn_instnorm_act_fwd(ptr(x), ptr(y), ptr(mean), ptr(rstd), n_inst, S, EPS, slope, ptr(ws), nbytes, stream(x))
    assert rc == 0, rc
    return y, mean, rstd


def in_bwd_c(x, mean, rstd, gy, slope, channels=None, gbs=0):
    n_inst, S = x.shape
    gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    assert gx.data_ptr() % 16 == 0
    nbytes = lib().dn_instnorm_workspace_bytes(n_inst, S)
    ws = workspace(nbytes, x.device)
    rc = lib().dn_instnorm_act_bwd(ptr(x), ptr(mean), ptr(rstd), ptr(gy), ptr(gx), n_inst, S, slope, channels or n_inst, gbs, ptr(ws), nbytes,
                                   stream(x))
    assert rc == 0, rc
    return gx


@pytest.mark.gpu
@pytest.mark.parametrize("shape,first,expect,slopes", IN_ROWS, ids=IN_IDS)
def test_instnorm_seams_c_abi_and_module(shape, first, expect, slopes):
    from diffnet_amd.networks.fused import InstanceNormAct
    n_inst, S = in_sizes(shape)
    x, gy, x64, mu, r = in_problem(n_inst, S, first)
    xd, gd = x.to(dev()), gy.to(dev())
    assert xd.data_ptr() % 16 == 0 and gd.data_ptr() % 16 == 0
    for slope in slopes:
        case = f"{'x'.join(map(str, shape))} slope={slope}"
        y, mean, rstd = in_fwd_c(xd, slope)
        gx = in_bwd_c(xd, mean, rstd, gd, slope)
        check("instnorm_fwd", case, **in_fwd_parts(y, mean, rstd, x64, mu, r, slope))
        check("instnorm_bwd", case, **in_bwd_parts(gx, x64, gy, mean, rstd, slope))
        # the module: the same launches on equally aligned tensors -> the same bits
        xm = xd.view(shape).requires_grad_(True)
        ym = InstanceNormAct(shape[1], slope=slope, eps=EPS)(xm)
        (gxm,) = torch.autograd.grad(ym, xm, gd.view(shape))
        assert ym.shape == tuple(shape) and torch.equal(ym.detach().reshape(y.shape), y), case
        assert torch.equal(gxm.reshape(gx.shape), gx), case


IN_OFF = [((2, 3, 32, 32), 1), ((1, 2, 128, 128), 1), ((1, 3, 3, 11, 31), 0)]       # float4 one pass, float4 sliced, scalar anyway (S = 1023)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["x", "cotangent"])
@pytest.mark.parametrize("shape,first", IN_OFF, ids=["x".join(map(str, s)) for s, _ in IN_OFF])
def test_instnorm_views_one_float_off(shape, first, which):
    """a misaligned x or cotangent takes the scalar path: within the bounds, and bitwise the aligned result where that is scalar as well"""
    from diffnet_amd.networks.fused import InstanceNormAct
    n_inst, S = in_sizes(shape)
    x, gy, x64, mu, r = in_problem(n_inst, S, first)
    xa, ga = x.to(dev()), gy.to(dev())
    xo, go = (one_float_off(xa), ga) if which == "x" else (xa, one_float_off(ga))
    assert (xo.data_ptr() | go.data_ptr()) % 16 == 4 and (xa.data_ptr() | ga.data_ptr()) % 16 == 0
    slope = 0.2
    case = f"{'x'.join(map(str, shape))} {which} one float off"
    y, mean, rstd = in_fwd_c(xo, slope)
    gx = in_bwd_c(xo, mean, rstd, go, slope)
    check("instnorm_off", case, **in_fwd_parts(y, mean, rstd, x64, mu, r, slope), **in_bwd_parts(gx, x64, gy, mean, rstd, slope))
    ya, ma, ra = in_fwd_c(xa, slope)
    gxa = in_bwd_c(xa, ma, ra, ga, slope)
    if S % 4 != 0:                                                     # scalar in both runs: the same order of every sum
        assert torch.equal(y, ya) and torch.equal(mean, ma) and torch.equal(rstd, ra) and torch.equal(gx, gxa), case
    elif which == "cotangent":                                         # the forward never saw the cotangent
        assert torch.equal(y, ya) and torch.equal(mean, ma) and torch.equal(rstd, ra), case
    # through the module: the views reach the kernels as they are
    xm = xo.view(shape).requires_grad_(True)
    ym = InstanceNormAct(shape[1], slope=slope, eps=EPS)(xm)
    (gxm,) = torch.autograd.grad(ym, xm, go.view(shape))
    assert torch.equal(ym.detach().reshape(y.shape), y) and torch.equal(gxm.reshape(gx.shape), gx), case


@pytest.mark.gpu
def test_instnorm_channel_slice_cotangent_sliced_path():
    """the cotangent is wide[:, 1 : 1 + C] of a (B, 2 C, ...) tensor, read in place through its batch stride; S = 65540, 8 slices"""
    from diffnet_amd.networks.fused import InstanceNormAct
    shape, slope = (2, 2, 4, 16385), 0.2
    (B, Cn), (n_inst, S) = shape[:2], in_sizes(shape)
    assert in_nchunk(n_inst, S) == 8
    x, gy, x64, mu, r = in_problem(n_inst, S, 0)
    xd = x.to(dev())
    wide = randn((B, 2 * Cn) + shape[2:], "wide").to(dev())
    wide[:, 1:1 + Cn] = gy.view(shape).to(dev())
    cot = wide[:, 1:1 + Cn]
    assert not cot.is_contiguous() and cot.stride(0) == 2 * Cn * S and cot.data_ptr() % 16 == 0
    y, mean, rstd = in_fwd_c(xd, slope)
    gx = in_bwd_c(xd, mean, rstd, cot, slope, channels=Cn, gbs=cot.stride(0))
    check("instnorm_bwd", "2x2x4x16385 channel slice", **in_bwd_parts(gx, x64, gy, mean, rstd, slope))
    assert torch.equal(gx, in_bwd_c(xd, mean, rstd, gy.to(dev()), slope)), "the same sums in the same order as from a contiguous cotangent"
    xm = xd.view(shape).requires_grad_(True)
    (gxm,) = torch.autograd.grad(InstanceNormAct(Cn, slope=slope, eps=EPS)(xm), xm, cot)
    assert torch.equal(gxm.reshape(gx.shape), gx)


# ---------------------------------------------------------------------------------------------
# 3. output blocks
# ---------------------------------------------------------------------------------------------
def uc_fwd_c(x, w, b, act):
    """x (B, C, *sp), w (C, K, ..), b (1) or None on the GPU -> (B, 1, *2 sp) through the C ABI"""
    nd, (B, C) = x.dim() - 2, x.shape[:2]
    out = torch.empty((B, 1) + tuple(2 * s for s in x.shape[2:]), dtype=torch.float32, device=x.device)
    sizes, fwd = ((lib().dn_upconv_out_workspace_bytes, lib().dn_upconv_out_fwd) if nd == 2 else
                  (lib().dn_upconv3d_out_workspace_bytes, lib().dn_upconv3d_out_fwd))
    nbytes = sizes(B, C, *x.shape[2:])
    ws = workspace(nbytes, x.device)
    rc = fwd(ptr(x), ptr(w), ptr(b), ptr(out), B, C, *x.shape[2:], act, ptr(ws), nbytes, stream(x))
    assert rc == 0, rc
    return out


def uc_bwd_c(x, w, out, gout, act, want=(True, True, True)):
    nd, (B, C) = x.dim() - 2, x.shape[:2]
    gx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want[0] else None
    gw = torch.empty(w.shape, dtype=torch.float32, device=x.device) if want[1] else None
    gb = torch.empty(1, dtype=torch.float32, device=x.device) if want[2] else None
    sizes, bwd = ((lib().dn_upconv_out_workspace_bytes, lib().dn_upconv_out_bwd) if nd == 2 else
                  (lib().dn_upconv3d_out_workspace_bytes, lib().dn_upconv3d_out_bwd))
    nbytes = sizes(B, C, *x.shape[2:])
    ws = workspace(nbytes, x.device)
    rc = bwd(ptr(x), ptr(w), ptr(out), ptr(gout), ptr(gx), ptr(gw), ptr(gb), B, C, *x.shape[2:], act, ptr(ws), nbytes, stream(x))
    assert rc == 0, rc
    return gx, gw, gb


def n_uc(nd, C, tpw=1, gz=3):
    """roundings per family (module docstring); gz = 0 when the cotangent is used as it is (act = 0)"""
    return dict(fwd=C + 14 if nd == 2 else 8 * C + 9, gx=(29 if nd == 2 else 72) + gz, gw=128 * tpw + 5 + gz, gb=tpw + (5 if nd == 2 else 6) + gz)


EXACT = [(2, 3, 5, 65), (1, 2, 1, 1), (1, 2, 3, 5, 65), (1, 1, 1, 1, 1)]


def one_hot_weight(C, K, nd, c0, tap):
    w = torch.zeros((C,) + (K,) * nd)
    w[(c0,) + tap] = 1.0
    return w


def first_difference(got, want):
    idx = (got != want).nonzero()[0].tolist()
    return f"first difference at (sample, channel, position) {idx}: got {got[tuple(idx)].item()!r}, gather {want[tuple(idx)].item()!r}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", EXACT, ids=["x".join(map(str, s)) for s in EXACT])
def test_output_block_single_tap_is_an_exact_gather(shape):
    nd, C = len(shape) - 2, shape[1]
    K = R.block_geometry(nd)[0]
    x = randn(shape, "exact x", shape)
    g = randn((shape[0], 1) + tuple(2 * s for s in shape[2:]), "exact g", shape)
    xd, gd = x.to(dev()), g.to(dev())
    for n, tap in enumerate(itertools.product(range(K), repeat=nd)):
        c0 = n % C
        wd = one_hot_weight(C, K, nd, c0, tap).to(dev())
        z = uc_fwd_c(xd, wd, None, 0).cpu()
        want = R.upconv_gather(x, c0, tap, nd)
        assert torch.equal(z, want), f"forward {shape} channel {c0} tap {tap}: " + first_difference(z, want)
        gx, _, _ = uc_bwd_c(xd, wd, None, gd, 0, want=(True, False, False))
        want = R.upconv_gather_adjoint(g, C, c0, tap, nd)
        assert torch.equal(gx.cpu(), want), f"input gradient {shape} channel {c0} tap {tap}: " + first_difference(gx.cpu(), want)


def uc_inputs(shape, *key):
    nd, C = len(shape) - 2, shape[1]
    K = R.block_geometry(nd)[0]
    x = randn(shape, "uc x", shape, *key)
    if C >= 2:
        x[:, C - 1] = 0.0                  # a channel without a term: its weight gradient has A = 0 and must be exactly 0
    return x, 0.5 * randn((C,) + (K,) * nd, "uc w", shape, *key), 0.5 * randn((1,), "uc b", shape, *key)


@functools.lru_cache(maxsize=1)
def uc_bwd_problem(shape):
    """float32 x, w, a given out in (0, 1) and gout; float64 gradients of sum(z gz), gz = gout y (1 - y), and their magnitude fields"""
    nd = len(shape) - 2
    x, w, _ = uc_inputs(shape, "bwd")
    oshape = (shape[0], 1) + tuple(2 * s for s in shape[2:])
    out, gout = 0.05 + 0.9 * rand(oshape, "uc out", shape), randn(oshape, "uc gout", shape)
    o64 = out.double()
    ref = R.upconv_bwd(x.double(), w.double(), gout.double() * o64 * (1 - o64), nd)
    A = R.upconv_bwd(x.abs().double(), w.abs().double(), gout.abs().double() * o64 * (1 - o64), nd)
    return x, w, out, gout, ref, A


@pytest.mark.gpu
@pytest.mark.parametrize("shape,off,expect", UC2_ROWS + UC3_ROWS, ids=UC_IDS(UC2_ROWS + UC3_ROWS))
def test_output_block_backward_seams(shape, off, expect):
    nd, C = len(shape) - 2, shape[1]
    x, w, out, gout, ref, A = uc_bwd_problem(shape)
    tpw = uc_plan(shape)[2]
    assert tpw == expect[0]
    xd = one_float_off(x.to(dev())) if off else x.to(dev())
    assert xd.data_ptr() % 16 == (4 if off else 0)
    wd, od, gd = w.to(dev()), out.to(dev()), gout.to(dev())
    gx, gw, gb = uc_bwd_c(xd, wd, od, gd, 1)
    n = n_uc(nd, C, tpw)
    check(f"upconv{nd}d_bwd", "x".join(map(str, shape)) + (" in one float off" if off else ""),
          gx=(gx, ref[0], A[0], n["gx"]), gw=(gw, ref[1], A[1], n["gw"]), gb=(gb, ref[2], A[2], n["gb"]))
    if C >= 2:
        assert bool((A[1][C - 1] == 0).all()) and bool((gw[C - 1] == 0).all())
    if tpw > 1:                                     # fixed order: bitwise repeatable, and the same without the input gradient
        _, gw2, gb2 = uc_bwd_c(xd, wd, od, gd, 1, want=(False, True, True))
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
        _, gw3, _ = uc_bwd_c(xd, wd, od, gd, 1, want=(False, True, False))
        assert torch.equal(gw, gw3)


UC_SMALL = [(2, 3, 5, 65), (1, 2, 1, 1), (2, 70, 16, 16), (1, 65, 7, 9), (1, 2, 3, 5, 65), (1, 1, 1, 1, 1), (1, 33, 3, 4, 66), (2, 31, 2, 2, 2)]


@functools.lru_cache(maxsize=1)
def uc_fwd_problem(shape, cout):
    nd = len(shape) - 2
    xs, ws, bs = zip(*(uc_inputs(shape, "fwd", co) for co in range(cout)))
    x, w, b = xs[0], torch.stack(ws), torch.cat(bs)
    cot = randn((shape[0], cout) + tuple(2 * s for s in shape[2:]), "uc cot", shape, cout)
    x64 = x.double()
    z = [R.upconv(x64, w[co].double(), b[co].double(), nd) for co in range(cout)]
    Az = [R.upconv(x64.abs(), w[co].abs().double(), b[co].abs().double(), nd) for co in range(cout)]
    z0 = [R.upconv(x64, w[co].double(), None, nd) for co in range(cout)]
    Az0 = [R.upconv(x64.abs(), w[co].abs().double(), None, nd) for co in range(cout)]
    g = [R.upconv_bwd(x64, w[co].double(), cot[:, co:co + 1].double(), nd) for co in range(cout)]
    Ag = [R.upconv_bwd(x64.abs(), w[co].abs().double(), cot[:, co:co + 1].abs().double(), nd) for co in range(cout)]
    cat = lambda parts, k=None: torch.cat([p if k is None else p[k] for p in parts], 1 if k is None else 0)      # noqa: E731
    ref = dict(z=cat(z), z0=cat(z0), gx=sum(p[0] for p in g), gw=torch.stack([p[1] for p in g]), gb=cat(g, 2))
    mag = dict(z=cat(Az), z0=cat(Az0), gx=sum(p[0] for p in Ag), gw=torch.stack([p[1] for p in Ag]), gb=cat(Ag, 2))
    return x, w, b, cot, ref, mag


@pytest.mark.gpu
@pytest.mark.parametrize("cout", [1, 2])
@pytest.mark.parametrize("shape", UC_SMALL, ids=["x".join(map(str, s)) for s in UC_SMALL])
def test_output_block_functions_without_sigmoid(shape, cout):
    """upsample_pad_conv4 / upsample_conv3 with sigmoid=False: forward with and without bias, all gradients, and each of
    needs_input_grad = x only, weight only, bias only; cout = 2 runs one launch set per output channel and adds the input gradients"""
    from diffnet_amd.networks.fused import upsample_conv3, upsample_pad_conv4
    nd, C = len(shape) - 2, shape[1]
    fn = upsample_pad_conv4 if nd == 2 else upsample_conv3
    x, w, b, cot, ref, mag = uc_fwd_problem(shape, cout)
    n = n_uc(nd, C, 1, gz=0)
    n_gx = n["gx"] + cout - 1                                 # the per-channel input gradients are added by autograd: cout - 1 more roundings
    case = "x".join(map(str, shape)) + f" cout={cout}"
    cd = cot.to(dev())
    xd, wd, bd = (t.to(dev()).requires_grad_(True) for t in (x, w, b))
    z = fn(xd, wd, bd, sigmoid=False)
    gx, gw, gb = torch.autograd.grad(z, [xd, wd, bd], cd)
    z0 = fn(xd, wd, None, sigmoid=False)
    gx0, gw0 = torch.autograd.grad(z0, [xd, wd], cd)
    check(f"upconv{nd}d_fwd", case, z=(z, ref["z"], mag["z"], n["fwd"]), z_nobias=(z0, ref["z0"], mag["z0"], n["fwd"]))
    check(f"upconv{nd}d_bwd", case, gx=(gx, ref["gx"], mag["gx"], n_gx), gw=(gw, ref["gw"], mag["gw"], n["gw"]), gb=(gb, ref["gb"], mag["gb"], n["gb"]))
    assert torch.equal(gx0, gx) and torch.equal(gw0, gw), case + ": the gradients do not depend on the bias"
    for k, name in enumerate(("x", "weight", "bias")):
        leaves = [t.detach().clone().requires_grad_(k == i) for i, t in enumerate((xd, wd, bd))]
        (g1,) = torch.autograd.grad(fn(*leaves, sigmoid=False), leaves[k], cd)
        assert torch.equal(g1, (gx, gw, gb)[k]), f"{case}: needs_input_grad = {name} only"


SIGMOID = [(2, 3, 37, 65), (1, 2, 9, 10, 65)]


@functools.lru_cache(maxsize=2)
def sigmoid_problem(shape):
    """weights and bias scaled so that the float64 z spans [-20, 20] (its largest |z| is 20)"""
    nd = len(shape) - 2
    x, w, b = uc_inputs(shape, "sigmoid")
    z = R.upconv(x.double(), w.double(), b.double(), nd)
    s = 20.0 / float(z.abs().max())
    return x, (w.double() * s).float(), (b.double() * s).float(), z * s


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SIGMOID, ids=["x".join(map(str, s)) for s in SIGMOID])
def test_output_block_sigmoid_against_float64_of_the_same_sum(shape):
    x, w, b, z64 = sigmoid_problem(shape)
    xd, wd, bd = x.to(dev()), w.to(dev()), b.to(dev())
    z = uc_fwd_c(xd, wd, bd, 0).double().cpu()
    y = uc_fwd_c(xd, wd, bd, 1).double().cpu()
    assert float(z.min()) < -15 and float(z.max()) > 15, (float(z.min()), float(z.max()))
    s = torch.sigmoid(z)
    e = float(((y - s).abs() / (U * s * (1 + (1 - s) * (1 + z.abs())))).max())
    RATIOS["sigmoid_e"] = max(RATIOS.get("sigmoid_e", 0.0), e)
    print(f"layer-ratio sigmoid {'x'.join(map(str, shape))}: e={e:.3g} cap={SIGMOID_CAP} z in [{float(z.min()):.3g}, {float(z.max()):.3g}]")
    assert bool(((y >= 0) & (y <= 1)).all())
    assert e <= SIGMOID_CAP, f"sigmoid error {e:.3g} u s (1 + (1 - s)(1 + |z|)) exceeds the cap {SIGMOID_CAP}"


# ---------------------------------------------------------------------------------------------
# 4. stride-1 valid convolution
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cv_problem(B, Ci, Co, H, W, K):
    key = (B, Ci, Co, H, W, K)
    x, w, b = randn((B, Ci, H, W), "cv x", key), 0.5 * randn((Co, Ci, K, K), "cv w", key), randn((Co,), "cv b", key)
    gy = randn((B, Co, H - K + 1, W - K + 1), "cv gy", key)
    d = lambda t: t.double()          # noqa: E731
    a = lambda t: t.abs().double()    # noqa: E731
    ref = (R.conv_valid(d(x), d(w), d(b)), R.conv_valid(d(x), d(w), None)) + R.conv_valid_bwd(d(x), d(w), d(gy))
    mag = (R.conv_valid(a(x), a(w), a(b)), R.conv_valid(a(x), a(w), None)) + R.conv_valid_bwd(a(x), a(w), a(gy))
    return x, w, b, gy, ref, mag


def n_cv(Ci, Co, K):
    return dict(y=Ci * K * K + 1, gx=Co * K * K, gw=2, gb=2)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Ci,Co,H,W,K,bias", CV_ROWS, ids=CV_IDS)
def test_conv2d_valid_edges(B, Ci, Co, H, W, K, bias):
    from diffnet_amd.networks.fused import Conv2dValid
    x, w, b, gy, ref, mag = cv_problem(B, Ci, Co, H, W, K)
    n = n_cv(Ci, Co, K)
    m = Conv2dValid(Ci, Co, K, bias=bias).to(dev())
    with torch.no_grad():
        m.weight.copy_(w)
        if bias:
            m.bias.copy_(b)
    xd = x.to(dev()).requires_grad_(True)
    y = m(xd)
    assert y.shape == (B, Co, H - K + 1, W - K + 1)
    y.backward(gy.to(dev()))
    k = 0 if bias else 1
    parts = dict(y=(y, ref[k], mag[k], n["y"]), gx=(xd.grad, ref[2], mag[2], n["gx"]), gw=(m.weight.grad, ref[3], mag[3], n["gw"]))
    if bias:
        parts["gb"] = (m.bias.grad, ref[4], mag[4], n["gb"])
    check("conv2d_valid", "x".join(map(str, (B, Ci, Co, H, W, K))) + ("" if bias else " no bias"), **parts)
    if not bias:
        # no bias gradient comes back, and the weight gradient is bitwise the one of the call with a bias
        from diffnet_amd.networks.fused import _Conv2dValid

        class Ctx:                                                     # what autograd hands to backward, with every gradient asked for
            saved_tensors, has_bias, needs_input_grad = (xd.detach(), m.weight.detach()), False, (True, True, True)

        _, gw_fn, gb_fn = _Conv2dValid.backward(Ctx, gy.to(dev()))
        assert m.bias is None and gb_fn is None and torch.equal(gw_fn, m.weight.grad)
        gw_only = torch.empty_like(m.weight)
        gw_both, gb_both = torch.empty_like(m.weight), torch.empty(Co, dtype=torch.float32, device=dev())
        gd = gy.to(dev())
        for gw_, gb_ in ((gw_only, None), (gw_both, gb_both)):
            rc = lib().dn_conv2d_valid_bwd_weight(ptr(xd.detach()), ptr(gd), ptr(gw_), ptr(gb_), B, Ci, Co, H, W, K, stream(gd))
            assert rc == 0, rc
        assert torch.equal(gw_only, gw_both) and torch.equal(gw_only, m.weight.grad)
        check("conv2d_valid", "bias gradient next to it", gb=(gb_both, ref[4], mag[4], n["gb"]))


# ---------------------------------------------------------------------------------------------
# CPU: the bounds have teeth
# ---------------------------------------------------------------------------------------------
def in_emulate32(x, gy, slope):
    """the kernels' float32 steps with exact statistics: y, mean, rstd, gx"""
    mu, r = R.instnorm_stats(x.double(), EPS64)
    m, r = mu.float(), r.float()
    h = (x - m) * r
    g = gy * torch.where(h > 0, torch.ones_like(h), torch.full_like(h, slope))
    mg, mgx = g.double().mean(1, keepdim=True).float(), (g.double() * h.double()).mean(1, keepdim=True).float()
    return R.act(h, slope), m, r, r * (g - mg - h * mgx)


@pytest.mark.parametrize("slope", ALL_SLOPES)
@pytest.mark.parametrize("S", [2, 63, 1028, 16385])
def test_instnorm_bounds_pass_float32_and_reject_wrong_statistics(S, slope):
    n_inst = 8
    x = in_data(n_inst, S, 0, "teeth")
    gy = randn((n_inst, S), "teeth gy", S)
    x64 = x.double()
    mu, r = R.instnorm_stats(x64, EPS64)
    y, m, r32, gx = in_emulate32(x, gy, slope)
    ok = check("cpu_float32", f"instnorm S={S} slope={slope}", **in_fwd_parts(y, m, r32, x64, mu, r, slope), **in_bwd_parts(gx, x64, gy, m, r32, slope))
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    parts = in_fwd_bound(x64, mu, r, slope)
    r_unbiased = 1.0 / torch.sqrt(var * S / (S - 1) + EPS64)                           # S - 1 in the variance
    bad = {"S - 1": bound_ratio(R.instnorm_fwd(x64, mu, r_unbiased, slope)[0], *parts),
           "S - 1 rstd": bound_ratio(r_unbiased, r, r, STAT_N)}
    tiny = slice(2, None, 4)                                                           # the tiny-spread instances: var 1e-6 against eps 1e-5
    r_noeps = 1.0 / torch.sqrt(var[tiny])
    bad["eps dropped"] = bound_ratio(R.instnorm_fwd(x64[tiny], mu[tiny], r_noeps, slope)[0], *(p[tiny] if torch.is_tensor(p) else p for p in parts))
    if slope != 1.0:
        ref, A = R.instnorm_bwd(x64, gy.double(), m.double(), r32.double(), slope)
        bad["mean(g h) without act'"] = bound_ratio(R.instnorm_bwd(x64, gy.double(), m.double(), r32.double(), slope, act_derivative=False)[0], ref, A, 9)
    print("exact float64 evaluations of the wrong operator:", {k: f"{v:.3g}" for k, v in bad.items()}, "against", {k: f"{v:.3g}" for k, v in ok.items()})
    for k, v in bad.items():
        assert v > 10.0, f"{k}: the bound does not notice ({v:.3g})"


def test_instnorm_rstd_bound_rejects_unshifted_sums():
    """what the kernel did before this suite: float64 sums of x and x^2 in lane-strided order, var = E[x^2] - mu^2, on the large-mean data"""
    S = 16380
    x64 = (1000.0 + 0.01 * randn((1, S), "unshifted")).double()
    mu, r = R.instnorm_stats(x64, EPS64)
    lanes = F.pad(x64, (0, -S % 256)).reshape(-1, 256)
    s, q = torch.zeros(256, dtype=torch.float64), torch.zeros(256, dtype=torch.float64)
    for row in lanes:
        s, q = s + row, q + row * row
    m1 = s.sum() / S
    r1 = 1.0 / torch.sqrt((q.sum() / S - m1 * m1).clamp_min(0.0) + EPS64)
    v = bound_ratio(r1.float().reshape(1, 1), r, r, STAT_N)
    d = lanes - x64[0, 0]
    d[-1, S % 256:] = 0.0
    s, q = torch.zeros(256, dtype=torch.float64), torch.zeros(256, dtype=torch.float64)
    for row in d:
        s, q = s + row, q + row * row
    m2 = s.sum() / S
    r2 = 1.0 / torch.sqrt((q.sum() / S - m2 * m2).clamp_min(0.0) + EPS64)
    v2 = bound_ratio(r2.float().reshape(1, 1), r, r, STAT_N)
    print(f"rstd error / bound: sums of x and x^2 {v:.3g}, sums of x - x[0] {v2:.3g}")
    assert v > 10.0 and v2 <= 1.0


def torch_block(x, w, b, nd, pad=(1, 0, 1, 0)):
    """the stock composition the reference networks use, in the dtype of the arguments"""
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    if nd == 2:
        return F.conv2d(F.pad(up, pad), w[None], b, padding=1)
    return F.conv3d(up, w[None], b, padding=1)


@pytest.mark.parametrize("shape", [(2, 3, 5, 65), (1, 2, 3, 5, 9)], ids=["2d", "3d"])
def test_output_block_bounds_pass_float32_and_reject_index_errors(shape):
    nd, C = len(shape) - 2, shape[1]
    x, w, b, cot, ref, mag = uc_fwd_problem(shape, 1)
    n = n_uc(nd, C, 1, gz=0)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w[0], b))
    z = torch_block(xr, wr, br, nd)
    gx, gw, gb = torch.autograd.grad(z, [xr, wr, br], cot)
    ok = check("cpu_float32", f"upconv{nd}d", z=(z, ref["z"], mag["z"], n["fwd"]), gx=(gx, ref["gx"], mag["gx"], n["gx"]),
               gw=(gw[None], ref["gw"], mag["gw"], n["gw"]), gb=(gb, ref["gb"], mag["gb"], n["gb"]))
    # the restatement in layers_ref is the stock composition: float64 against float64, at rounding level
    z64 = torch_block(x.double(), w[0].double(), b.double(), nd)
    assert bound_ratio(z64, ref["z"], mag["z"], 2.0 ** -20) <= 1.0
    x64, w64, b64 = x.double(), w[0].double(), b.double()
    K = R.block_geometry(nd)[0]
    bad = {"dropped tap": bound_ratio(R.upconv(x64, w64, b64, nd, skip_tap=(K - 1,) * nd), ref["z"], mag["z"], n["fwd"])}
    if nd == 2:
        bad["phases swapped"] = bound_ratio(R.swap_phases(ref["z"]), ref["z"], mag["z"], n["fwd"])
        bad["zero pad on the wrong side"] = bound_ratio(torch_block(x64, w64, b64, nd, pad=(0, 1, 0, 1)), ref["z"], mag["z"], n["fwd"])
        gzs = R.swap_phases(cot.double())
    else:
        gzs = torch.roll(cot.double(), 1, dims=-1)
    wrong = R.upconv_bwd(x64, w64, gzs, nd)
    bad["cotangent phases swapped / shifted: gx"] = bound_ratio(wrong[0], ref["gx"], mag["gx"], n["gx"])
    bad["cotangent phases swapped / shifted: gw"] = bound_ratio(wrong[1][None], ref["gw"], mag["gw"], n["gw"])
    print("exact float64 evaluations of the wrong operator:", {k: f"{v:.3g}" for k, v in bad.items()}, "against", {k: f"{v:.3g}" for k, v in ok.items()})
    for k, v in bad.items():
        assert v > 100.0, f"{k}: the bound does not notice ({v:.3g})"


@pytest.mark.parametrize("shape", EXACT, ids=["x".join(map(str, s)) for s in EXACT])
def test_stock_float32_modules_give_the_gathers_exactly(shape):
    nd, C = len(shape) - 2, shape[1]
    K = R.block_geometry(nd)[0]
    x = randn(shape, "exact x", shape)
    g = randn((shape[0], 1) + tuple(2 * s for s in shape[2:]), "exact g", shape)
    taps = list(itertools.product(range(K), repeat=nd))
    for n, tap in enumerate(taps):
        c0 = n % C
        w = one_hot_weight(C, K, nd, c0, tap)
        xr = x.clone().requires_grad_(True)
        z = torch_block(xr, w, None, nd)
        want = R.upconv_gather(x, c0, tap, nd)
        assert torch.equal(z.detach(), want), (shape, tap)
        # the adjoint adds up to 2^nd cotangent values: exact, whatever the order, in float64
        xr64 = x.double().requires_grad_(True)
        (gx64,) = torch.autograd.grad(torch_block(xr64, w.double(), None, nd), xr64, g.double())
        assert torch.equal(gx64, R.upconv_gather_adjoint(g.double(), C, c0, tap, nd)), (shape, tap)
        adj = R.upconv_gather_adjoint(g, C, c0, tap, nd)
        assert bound_ratio(adj, gx64, R.upconv_gather_adjoint(g.abs().double(), C, c0, tap, nd), 2 ** nd) <= 1.0
        if min(shape[2:]) > 1:                     # one row, one column or one tap off is another tensor
            other = taps[(n + 1) % len(taps)]
            assert not torch.equal(R.upconv_gather(x, c0, other, nd), want)
            assert not torch.equal(torch.roll(want, 1, dims=-1), want) and not torch.equal(torch.roll(want, 1, dims=-2), want)
            assert not torch.equal(R.upconv_gather_adjoint(g, C, c0, other, nd), adj)


@pytest.mark.parametrize("B,Ci,Co,H,W,K,bias", CV_ROWS, ids=CV_IDS)
def test_conv2d_valid_bounds_pass_float32_and_reject_a_flipped_kernel(B, Ci, Co, H, W, K, bias):
    x, w, b, gy, ref, mag = cv_problem(B, Ci, Co, H, W, K)
    n = n_cv(Ci, Co, K)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(xr, wr, br)
    gx, gw, gb = torch.autograd.grad(y, [xr, wr, br], gy)
    # torch's float32 weight gradient is a float32 sum over B Ho Wo positions, not the kernels' fp64 one: its own count
    npos = B * (H - K + 1) * (W - K + 1)
    check("cpu_float32", f"conv2d_valid {(B, Ci, Co, H, W, K)}", y=(y, ref[0], mag[0], n["y"]), gx=(gx, ref[2], mag[2], n["gx"]),
          gw=(gw, ref[3], mag[3], npos + 1), gb=(gb, ref[4], mag[4], npos + 1))
    if K > 1 and H > K:
        flipped = R.conv_valid(x.double(), w.double().flip(-1, -2), b.double())          # correlation taken for convolution
        assert bound_ratio(flipped, ref[0], mag[0], n["y"]) > 100.0
        wrong = R.conv_valid_bwd(x.double(), w.double().flip(-1, -2), gy.double())
        assert bound_ratio(wrong[0], ref[2], mag[2], n["gx"]) > 100.0
