"""Plain restatements of the network-layer kernels (csrc/instnorm_act.hip, upconv_out.hip, upconv3d_out.hip, conv2d_direct.hip) for
tests/test_gpu_layer_seams.py, written from the layers' definitions and independent of the kernels' effective-weight tables: slices,
products and sums in the dtype of the arguments (float64 for a reference; applied to absolute values they give the magnitude field A
of a derived bound).  No convolution routine is called here: the output blocks are sums over taps of shifted slices of the upsampled,
zero-padded input, so a float64 reference of 162^3 outputs needs no im2col buffer."""
import itertools

import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------
# InstanceNorm (biased variance, eps) + leaky activation on (n_inst, S)
# ---------------------------------------------------------------------------------------------
def instnorm_stats(x, eps):
    """two-pass mean and 1 / sqrt(var + eps) per row, in x's dtype"""
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return mu, 1.0 / torch.sqrt(var + eps)


def act(t, slope):
    return torch.where(t > 0, t, slope * t)


def instnorm_fwd(x, mu, r, slope):
    """y and the normalised value t = (x - mu) r"""
    t = (x - mu) * r
    return act(t, slope), t


def instnorm_bwd(x, gy, m, r, slope, act_derivative=True):
    """gx = r (g - mean g - h mean(g h)), g = gy act'(h), h = (x - m) r, and its magnitude field r (|g| + mean|g| + |h| mean|g h|).
    act_derivative=False leaves act' out of the second mean only (a mutation for the teeth test)."""
    h = (x - m) * r
    g = gy * torch.where(h > 0, torch.ones_like(h), torch.full_like(h, slope))
    gh = (g if act_derivative else gy) * h
    ref = r * (g - g.mean(1, keepdim=True) - h * gh.mean(1, keepdim=True))
    A = r.abs() * (g.abs() + g.abs().mean(1, keepdim=True) + h.abs() * (g * h).abs().mean(1, keepdim=True))
    return ref, A


# ---------------------------------------------------------------------------------------------
# Output blocks: Upsample(x2, nearest) -> zero padding -> convolution to one channel
#   2-D: ZeroPad2d((1, 0, 1, 0)) + Conv2d(4 x 4, padding 1):  z[Y][X] = b + sum W[c][ky][kx] U[c][Y + ky - 2][X + kx - 2]
#   3-D: Conv3d(3 x 3 x 3, padding 1):                        z[Z][Y][X] = b + sum W[c][kz][ky][kx] U[c][Z + kz - 1][Y + ky - 1][X + kx - 1]
# ---------------------------------------------------------------------------------------------
def block_geometry(nd):
    """(taps per axis, zeros before, zeros after) of the nd-dimensional block"""
    return (4, 2, 1) if nd == 2 else (3, 1, 1)


def upsampled_padded(x, nd):
    K, lo, hi = block_geometry(nd)
    for ax in range(2, 2 + nd):
        x = x.repeat_interleave(2, dim=ax)
    return F.pad(x, (lo, hi) * nd)


def _window(t, tap, size):
    """t[..., tap_0 : tap_0 + size_0, tap_1 : ...] over the trailing axes"""
    return t[(Ellipsis,) + tuple(slice(k, k + n) for k, n in zip(tap, size))]


def _wtap(w, tap):
    """w (C, K, ..) at one tap as (1, C, 1, ..)"""
    nd = len(tap)
    return w[(slice(None),) + tuple(tap)].reshape((1, -1) + (1,) * nd)


def upconv(x, w, b, nd, skip_tap=None):
    """x (B, C, *sp), w (C, K, ..), b scalar tensor or None -> z (B, 1, *2 sp); skip_tap leaves one tap out (a mutation)"""
    K = block_geometry(nd)[0]
    U = upsampled_padded(x, nd)
    size = tuple(2 * s for s in x.shape[2:])
    z = torch.zeros((x.shape[0],) + size, dtype=x.dtype)
    for tap in itertools.product(range(K), repeat=nd):
        if tap != skip_tap:
            z += (_window(U, tap, size) * _wtap(w, tap)).sum(1)
    return (z if b is None else z + b).unsqueeze(1)


def upconv_bwd(x, w, gz, nd):
    """gradients of sum(z gz) wrt x, w and b"""
    K, lo, hi = block_geometry(nd)
    U = upsampled_padded(x, nd)
    size = tuple(gz.shape[2:])
    gw = torch.zeros_like(w)
    gU = torch.zeros_like(U)
    red = (0,) + tuple(range(2, 2 + nd))
    for tap in itertools.product(range(K), repeat=nd):
        gw[(slice(None),) + tap] = (_window(U, tap, size) * gz).sum(red)
        _window(gU, tap, size).add_(gz * _wtap(w, tap))
    gU = _window(gU, (lo,) * nd, size)
    shape = list(x.shape[:2])
    for s in x.shape[2:]:
        shape += [s, 2]
    gx = gU.reshape(shape).sum(tuple(range(3, 3 + 2 * nd, 2)))
    return gx, gw, gz.sum().reshape(1)


def upconv_gather(x, c0, tap, nd):
    """the forward block for a weight that is 1 at (c0, tap) and 0 elsewhere: one upsampled, zero-padded plane, shifted"""
    size = tuple(2 * s for s in x.shape[2:])
    return _window(upsampled_padded(x[:, c0:c0 + 1], nd), tap, size).clone()


def upconv_gather_adjoint(g, C, c0, tap, nd):
    """the input gradient for that weight: channel c0 collects, for each low-resolution cell, the cotangent at the 2^nd outputs that read
    it through `tap` -- added one after the other in row-major order of the output offset, from 0, which is the order of the kernels'
    fma chain (every other term of the chain is an exact zero) -- and every other channel is 0.  In float64 the order does not matter."""
    K, lo, hi = block_geometry(nd)
    sp = tuple(s // 2 for s in g.shape[2:])
    # low-resolution cell i is upsampled index 2 i + a, read by output 2 i + a - tap + lo
    gp = F.pad(g, (K, K) * nd)
    acc = torch.zeros((g.shape[0], 1) + sp, dtype=g.dtype)
    for off in itertools.product(range(-K, K + 2), repeat=nd):               # output offset relative to 2 i, row-major
        if all(0 <= o + t - lo <= 1 for o, t in zip(off, tap)):
            acc = acc + gp[(Ellipsis,) + tuple(slice(K + o, K + o + 2 * s, 2) for o, s in zip(off, sp))]
    out = torch.zeros((g.shape[0], C) + sp, dtype=g.dtype)
    out[:, c0:c0 + 1] = acc
    return out


def swap_phases(z):
    """2-D output with the two phase indices of every 2 x 2 block exchanged: new[2 i + a][2 j + b] = old[2 i + b][2 j + a]"""
    B, _, H, W = z.shape
    return z.reshape(B, 1, H // 2, 2, W // 2, 2).permute(0, 1, 2, 5, 4, 3).reshape(B, 1, H, W)


# ---------------------------------------------------------------------------------------------
# stride-1 valid convolution, K x K
# ---------------------------------------------------------------------------------------------
def conv_valid(x, w, b):
    B, Ci, H, W = x.shape
    Co, K = w.shape[0], w.shape[-1]
    size = (H - K + 1, W - K + 1)
    y = torch.zeros((B, Co) + size, dtype=x.dtype)
    for ky, kx in itertools.product(range(K), repeat=2):
        y += torch.einsum("bchw,oc->bohw", _window(x, (ky, kx), size), w[:, :, ky, kx])
    return y if b is None else y + b.reshape(1, -1, 1, 1)


def conv_valid_bwd(x, w, gy):
    K = w.shape[-1]
    size = tuple(gy.shape[2:])
    gx, gw = torch.zeros_like(x), torch.zeros_like(w)
    for ky, kx in itertools.product(range(K), repeat=2):
        _window(gx, (ky, kx), size).add_(torch.einsum("bohw,oc->bchw", gy, w[:, :, ky, kx]))
        gw[:, :, ky, kx] = torch.einsum("bohw,bchw->oc", gy, _window(x, (ky, kx), size))
    return gx, gw, gy.sum((0, 2, 3))
