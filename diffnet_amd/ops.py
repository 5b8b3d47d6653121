"""Torch-facing wrappers around the C ABI (include/diffnet_hip.h): device pointers + the current HIP
stream are handed to libdiffnet_hip.so; autograd.Function classes pair each forward kernel with
its adjoint kernel so user `loss()` bodies compose with ordinary torch ops.

No CPU fallback: every op requires fp32 CUDA(HIP) tensors and raises otherwise.
"""
import ctypes as C
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import DnCoefGradArgs, DnDirichlet, DnEikonalArgs, DnFdmPoissonArgs, DnFoslsArgs, DnFsdtArgs, DnHelmholtzArgs, DnMesh, DnNsArgs, DnPointsArgs, DnPoissonArgs, DnPoissonCgArgs, DnPoissonDiagArgs, DnStokesArgs, DnStrongformArgs, DnTransportArgs, I32x3, DiffNetHipError


def _require(t, name, ndim=None, strict=False):
    """`strict` (prepared launches): the tensor itself must be usable -- a hidden .contiguous() copy would be read by every later
    launch instead of the caller's (since updated) tensor."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise DiffNetHipError(f"{name} is on {t.device}: the FEM ops run on the GPU only (no CPU fallback); move it with .cuda()")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name} must have {ndim} dims, got shape {tuple(t.shape)}")
    if strict and not t.is_contiguous():
        raise DiffNetHipError(f"{name} is not contiguous: a prepared launch (PoissonPlan) keeps the pointers it was given; pass a contiguous tensor")
    return t.contiguous()


def _raw_stream(device):
    """The current HIP stream of `device` as an integer handle (torch.cuda.current_stream() builds a Stream object: ~8 us per call,
    more than the rest of a cached launch)."""
    return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())


def _stream(t):
    return C.c_void_p(_raw_stream(t.device))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------------------------
# generic gauss_pt_eval / assembly
# ------------------------------------------------------------------------------------------------
def _sizes_xyz(t, nsd):
    s = list(t.shape[2:])          # (z, y, x) order in memory
    s = s[::-1] + [1] * (3 - nsd)  # -> (x, y, z)
    return I32x3(*s)


def _gpe_fwd(x, tables, nsd, nbf, stride):
    x = _require(x, "tensor", nsd + 2)
    if x.shape[1] != 1:
        raise ValueError(f"gauss_pt_eval expects a single-channel field (B,1,...), got {tuple(x.shape)}")
    G = tables.shape[0]
    out_sp = [(n - nbf) // stride + 1 for n in x.shape[2:]]
    if min(out_sp) < 1:
        raise ValueError(f"field {tuple(x.shape)} smaller than the {nbf}-node element")
    out = torch.empty((x.shape[0], G, *out_sp), dtype=torch.float32, device=x.device)
    rc = _lib.lib().dn_gauss_pt_eval_fwd(_p(x), _p(tables), _p(out), x.shape[0], nsd, _sizes_xyz(x, nsd), nbf, stride, G, _stream(x))
    _lib.check(rc, "dn_gauss_pt_eval_fwd")
    return out


def _gpe_bwd(gout, tables, shape, nsd, nbf, stride):
    gout = _require(gout, "grad_output")
    gin = torch.empty(shape, dtype=torch.float32, device=gout.device)
    sizes = I32x3(*(list(shape[2:])[::-1] + [1] * (3 - nsd)))
    rc = _lib.lib().dn_gauss_pt_eval_bwd(_p(gout), _p(tables), _p(gin), shape[0], nsd, sizes, nbf, stride, tables.shape[0], _stream(gout))
    _lib.check(rc, "dn_gauss_pt_eval_bwd")
    return gin


class _GpeFn(torch.autograd.Function):
    """gauss_pt_eval in eager mode: the launch behind a plain autograd.Function (the registered operator's dispatch costs ~75 us of host time per
    call -- tools/bench_ops.py: 157 us for a forward + backward whose two kernels take 60 -- and an unchanged reference loss() makes eight such
    calls per step).  Linear: the backward is the adjoint operator, whose backward is this one again."""

    @staticmethod
    def forward(ctx, x, tables, nsd, nbf, stride):
        ctx.save_for_backward(tables)
        ctx.meta = (tuple(x.shape), nsd, nbf, stride)
        return _gpe_fwd(x, tables, nsd, nbf, stride)

    @staticmethod
    def backward(ctx, g):
        (tables,) = ctx.saved_tensors
        shape, nsd, nbf, stride = ctx.meta
        return _GaussPtEvalT.apply(g, tables, shape, nsd, nbf, stride), None, None, None, None


class _GpeTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gout, tables, shape, nsd, nbf, stride):
        ctx.save_for_backward(tables)
        ctx.meta = (nsd, nbf, stride)
        return _gpe_bwd(gout, tables, tuple(shape), nsd, nbf, stride)

    @staticmethod
    def backward(ctx, gg):
        (tables,) = ctx.saved_tensors
        nsd, nbf, stride = ctx.meta
        return _GaussPtEval.apply(gg, tables, nsd, nbf, stride), None, None, None, None, None


def _wants_grad(t):
    return torch.is_grad_enabled() and isinstance(t, torch.Tensor) and t.requires_grad


class _GaussPtEval:
    """`gauss_pt_eval`: linear in the field, its backward is the adjoint operator `_GaussPtEvalT`, whose backward is this one again --
    differentiable to any order like the reference's conv formulation.  Under torch.compile / torch.export the registered operator
    diffnet_mi::gauss_pt_eval_fwd (diffnet_amd/torch_ops.py: an ordinary graph node); in eager mode the same launch behind a plain
    autograd.Function, or directly when nothing requires a gradient."""

    @staticmethod
    def apply(x, tables, nsd, nbf, stride):
        if torch.compiler.is_compiling():
            from . import torch_ops
            return torch_ops.gauss_pt_eval_fwd(x, tables, nsd, nbf, stride)
        if _wants_grad(x):
            return _GpeFn.apply(x, tables, nsd, nbf, stride)
        return _gpe_fwd(x, tables, nsd, nbf, stride)


class _GaussPtEvalT:
    """Adjoint of `_GaussPtEval` (element / Gauss-point cotangents -> nodal field): diffnet_mi::gauss_pt_eval_bwd under torch.compile."""

    @staticmethod
    def apply(gout, tables, shape, nsd, nbf, stride):
        if torch.compiler.is_compiling():
            from . import torch_ops
            return torch_ops.gauss_pt_eval_bwd(gout, tables, list(shape), nsd, nbf, stride)
        if _wants_grad(gout):
            return _GpeTFn.apply(gout, tables, tuple(shape), nsd, nbf, stride)
        return _gpe_bwd(gout, tables, tuple(shape), nsd, nbf, stride)


def stack_tables(N, nsd):
    """(G, nbf^nsd) contiguous fp32 table from a list / ParameterList of (1,1,*nbf) kernels."""
    ts = [t.detach().reshape(-1) for t in N]
    return torch.stack(ts, 0).contiguous().float()


def gauss_pt_eval(tensor, N, nsd=2, stride=1):
    """Drop-in for DiffNet/DiffNetFEM.py:7-18 on the GPU: all len(N) Gauss-point channels in one launch.
    `N`: sequence of (1,1,*nbf) kernels, or an already stacked (G, nbf^nsd) tensor."""
    if nsd not in (1, 2, 3):
        raise UnboundLocalError("nsd must be 1, 2 or 3")   # the reference fails with UnboundLocalError here
    if isinstance(N, torch.Tensor) and N.dim() == 2:
        tables = N
        nbf = round(N.shape[1] ** (1.0 / nsd))
    else:
        nbf = N[0].shape[-1]
        tables = stack_tables(N, nsd)
    if tables.device != tensor.device:
        tables = tables.to(tensor.device)
    return _GaussPtEval.apply(tensor, tables, nsd, nbf, stride)


def _assemble_raw(r_split, nsd, nbf, base):
    r_split = _require(r_split, "R_split", nsd + 2)
    stride = nbf - 1
    if r_split.shape[1] != nbf ** nsd:
        raise ValueError(f"R_split must have {nbf ** nsd} local-basis channels, got {r_split.shape[1]}")
    node_sp = [n * stride + 1 for n in r_split.shape[2:]]
    if base is not None:
        out = _require(base, "Aglobal", nsd + 2).clone()
        if list(out.shape[2:]) != node_sp or out.shape[0] != r_split.shape[0]:
            raise ValueError("Aglobal shape does not match R_split")
    else:
        out = torch.empty((r_split.shape[0], 1, *node_sp), dtype=torch.float32, device=r_split.device)
    rc = _lib.lib().dn_assemble(_p(r_split), _p(out), r_split.shape[0], nsd, _sizes_xyz(out, nsd), nbf, stride,
                                1 if base is not None else 0, _stream(out))
    _lib.check(rc, "dn_assemble")
    return out


def _assemble_bwd_raw(gout, shape, nsd, nbf):
    gout = _require(gout, "grad_output")
    gs = torch.empty(shape, dtype=torch.float32, device=gout.device)
    rc = _lib.lib().dn_assemble_bwd(_p(gout), _p(gs), shape[0], nsd, _sizes_xyz(gout, nsd), nbf, nbf - 1, _stream(gout))
    _lib.check(rc, "dn_assemble_bwd")
    return gs


def assemble(r_split, nsd, nbf=2, out=None):
    """Element->node assembly (Q1_2D/3D_vector_assembly of the reference scripts, any degree):
    returns `out + scatter_add(r_split)` (out = zeros when omitted).  Deterministic gather form; registered operator
    diffnet_mi::assemble (linear: its backward is the per-element gather, whose backward is the assembly)."""
    if torch.compiler.is_compiling():
        from . import torch_ops
        return torch_ops.assemble(r_split, nsd, nbf) if out is None else torch_ops.assemble_onto(r_split, out, nsd, nbf)
    if _wants_grad(r_split) or _wants_grad(out):
        return _AssembleFn.apply(r_split, out, nsd, nbf)
    return _assemble_raw(r_split, nsd, nbf, out)


class _AssembleFn(torch.autograd.Function):
    """Assembly in eager mode (see _GpeFn): backward = the per-element gather, whose backward is the assembly again."""

    @staticmethod
    def forward(ctx, r_split, base, nsd, nbf):
        ctx.meta = (tuple(r_split.shape), nsd, nbf, base is not None)
        return _assemble_raw(r_split, nsd, nbf, base)

    @staticmethod
    def backward(ctx, g):
        shape, nsd, nbf, has_base = ctx.meta
        gr = _assemble_gather(g, shape, nsd, nbf) if ctx.needs_input_grad[0] else None
        return gr, (g if has_base and ctx.needs_input_grad[1] else None), None, None


class _AssembleGatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, shape, nsd, nbf):
        ctx.meta = (nsd, nbf)
        return _assemble_bwd_raw(g.contiguous(), tuple(shape), nsd, nbf)

    @staticmethod
    def backward(ctx, gg):
        nsd, nbf = ctx.meta
        return assemble(gg, nsd, nbf), None, None, None


def _assemble_gather(g, shape, nsd, nbf):
    if _wants_grad(g):
        return _AssembleGatherFn.apply(g, tuple(shape), nsd, nbf)
    return _assemble_bwd_raw(g.contiguous(), tuple(shape), nsd, nbf)


# ------------------------------------------------------------------------------------------------
# fused Poisson operator
# ------------------------------------------------------------------------------------------------
class Dirichlet:
    """u <- where(mask > 0.5, value, u); `value` a python float or a nodal field tensor."""

    def __init__(self, mask, value=0.0):
        self.mask = mask
        self.value = value


class PackedMask:
    """A Dirichlet mask held in HBM with ONE BIT per node (C ABI: DN_MASK_BITS, include/diffnet_hip.h) instead of the reference's
    fp32 image (`DiffNet/datasets/parametric/images.py:30`): 1/8 B per node in the loss instead of 4.  Build it once when the
    dataset is placed on the device: `PackedMask.pack(mask)` with mask (B|1, 1, *N) float32 / uint8 / bool on the GPU.  Usable
    wherever a mask is: the 2-D Q1 fused kernels read the bits directly, every other path gets the (cached) uint8 image."""

    def __init__(self, bits, shape):
        self.bits = bits                    # int32 (B, rows per sample, row_words)
        self.shape = tuple(shape)           # (B, 1, *N) of the image
        self._u8 = None

    @property
    def row_words(self):
        return int(self.bits.shape[-1])

    @staticmethod
    def pack(mask):
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
            raise DiffNetHipError("PackedMask.pack needs a CUDA tensor")
        m = mask.to(torch.uint8) if mask.dtype == torch.bool else mask
        if m.dtype not in (torch.float32, torch.uint8):
            raise TypeError("Dirichlet mask must be float32, uint8 or bool")
        m = m.contiguous()
        nx = m.shape[-1]
        rows = m.numel() // nx
        rw = (nx + 31) // 32
        bits = torch.empty((m.shape[0], rows // m.shape[0], rw), dtype=torch.int32, device=m.device)
        rc = _lib.lib().dn_pack_mask_bits(m.data_ptr(), _lib.MASK_U8 if m.dtype == torch.uint8 else _lib.MASK_F32, rows, nx, rw,
                                          bits.data_ptr(), _stream(m))
        _lib.check(rc, "dn_pack_mask_bits")
        return PackedMask(bits, m.shape)

    def image(self):
        """The uint8 image (B|1, 1, *N), unpacked once."""
        if self._u8 is None:
            out = torch.empty(self.shape, dtype=torch.uint8, device=self.bits.device)
            nx = self.shape[-1]
            rc = _lib.lib().dn_unpack_mask_bits(self.bits.data_ptr(), out.numel() // nx, nx, self.row_words, out.data_ptr(), _stream(out))
            _lib.check(rc, "dn_unpack_mask_bits")
            self._u8 = out
        return self._u8


class LoadVector:
    """The forcing of a sample as its ASSEMBLED load vector b_a = sum_e sum_g w_g N_a(g) f_g instead of nodal values f (include/diffnet_hip.h:
    dn_poisson_args.f_is_load).  The reference interpolates the nodal forcing to the Gauss points in every loss evaluation
    (IBN/poisson-2d/parametric/IBN_2D.py:128-130); the forcing of a sample does not change between training steps, so -- like
    `PackedMask.pack` for the Dirichlet masks -- it can be assembled ONCE when the dataset is placed on the device:
    `LoadVector.assemble(geom, f)`.  Passed as the `f` argument of energy_loss / energy_loss_and_grad / residual* / PoissonPlan; the
    kernel then spends one FMA per node on the forcing instead of the element arithmetic (3-D Q1 256^3: 114 -> 92 us).  Results equal
    the nodal-forcing call to rounding.  Taken by the 3-D Q1 two-element kernel only (even nx, 2-point rule, constant-value uint8 /
    float32 mask images); anything else raises DiffNetHipError (DN_E_UNSUPPORTED)."""

    def __init__(self, tensor):
        if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous()):
            raise DiffNetHipError("LoadVector needs a contiguous float32 CUDA tensor (B|1, 1, *N)")
        self.tensor = tensor
        self.shape = tensor.shape

    @staticmethod
    def assemble(geom, f):
        """b = (rule weights, no Jacobian factor) mass-type assembly of the nodal forcing f (B|1, 1, *N): one launch of the fused operator
        itself with u = 0 (out = -beta * b)."""
        if not (isinstance(f, torch.Tensor) and f.is_cuda):
            raise DiffNetHipError("LoadVector.assemble needs a CUDA tensor")
        f = f.detach().to(torch.float32).contiguous()
        zero = torch.zeros_like(f)
        out, _ = poisson_apply(geom, zero, None, f, None, (), alpha=0.0, beta=-1.0, c=0.0, wscale=1.0, out_scale=1.0, want_out=True, want_sums=False)
        return LoadVector(out)


class BoxFaces:
    """Dirichlet condition on faces of the domain box, derived from the geometry (C ABI: DN_MASK_BOX): no mask array is read at
    all.  The reference builds these masks as images (`IBN/poisson-2d/parametric/IBN_2D.py:69-73`, `rectangles.py:16,232-233`).
    faces: "all" or any of "xlo", "xhi", "ylo", "yhi", "zlo", "zhi" (x = last tensor axis)."""
    _BITS = {"xlo": _lib.FACE_XLO, "xhi": _lib.FACE_XHI, "ylo": _lib.FACE_YLO, "yhi": _lib.FACE_YHI, "zlo": _lib.FACE_ZLO, "zhi": _lib.FACE_ZHI}

    def __init__(self, faces="all"):
        if isinstance(faces, str):
            faces = list(self._BITS) if faces == "all" else [faces]
        self.bits = 0
        for f in faces:
            self.bits |= self._BITS[f]
        self._img = {}

    def image(self, node_shape, device):
        """The uint8 image (1, 1, *N) of the selected faces (cached per shape and device)."""
        key = (tuple(node_shape), str(device))
        img = self._img.get(key)
        if img is None:
            nsd = len(node_shape)
            img = torch.zeros((1, 1, *node_shape), dtype=torch.uint8, device=device)
            for ax, name in zip(range(nsd - 1, -1, -1), "xyz"):       # x is the last tensor axis
                idx = [slice(None)] * (nsd + 2)
                if self.bits & self._BITS[name + "lo"]:
                    idx[2 + ax] = 0; img[tuple(idx)] = 1
                if self.bits & self._BITS[name + "hi"]:
                    idx[2 + ax] = -1; img[tuple(idx)] = 1
            self._img[key] = img
        return img


def _mask_image(m, like):
    """Any mask form -> tensor image usable in torch.where against `like` (B,1,*N)."""
    if isinstance(m, PackedMask):
        return m.image()
    if isinstance(m, BoxFaces):
        return m.image(like.shape[2:], like.device)
    return m


# ---- mask images packed on first use (round 4) ------------------------------------------------------------------------------------
# The reference keeps Dirichlet masks as fp32 images and hands them to loss() every step (IBN_2D.py:69-73, 119-121); read as they are they
# cost the fused 2-D kernel 4 B per node and launch (72 against 54-56 us at 512^2 x 64), as uint8 images 1 B.  A one-shot call
# (energy_loss / energy_loss_and_grad / residual*) therefore packs a mask image to one bit per node the FIRST time it sees it and finds the
# bits again on later calls: the cache is keyed on the mask's storage (address, offset, shape, strides, dtype) and the current stream (an
# entry packed on one stream is not read by launches on another, which are not ordered behind the pack) AND checked against the mask's
# version counter -- an in-place write to the mask (or to any view of its storage) changes the version and the image is packed again -- and
# an entry holds the mask tensor itself, so that the address cannot be handed to another tensor while the entry lives.  Masks without a
# version counter (inference tensors, made under torch.inference_mode()) are not packed: the call reads the image.  LIMIT: writes that
# bypass autograd's version counter -- through `mask.data`, DLPack / CuPy views, or a kernel writing the storage by pointer -- are not seen,
# and the stale bits are used; after such a write call `call_cache_clear()` (or pack explicitly).  Small LRU; `AUTO_PACK_MASKS = False`
# turns it off.  Prepared launches (PoissonPlan) take what they are given: pack explicitly with PackedMask.pack there.
AUTO_PACK_MASKS = True
_PACK_CACHE = __import__("collections").OrderedDict()
_PACK_CACHE_MAX = 8
_PACK_STATS = {"hit": 0, "pack": 0}


def _version_of(m):
    """The tensor's version counter, None where it has none (inference tensors raise on the read)."""
    if m.is_inference():
        return None
    try:
        return m._version
    except RuntimeError:
        return None


def _packed_on_first_use(m):
    """The cached PackedMask of image `m`, packed now if needed; None where the image cannot be tracked (no version counter)."""
    ver = _version_of(m)
    if ver is None:
        return None
    key = (m.untyped_storage().data_ptr(), m.storage_offset(), tuple(m.shape), tuple(m.stride()), m.dtype, _raw_stream(m.device))
    with _WS_LOCK:
        ent = _PACK_CACHE.get(key)
        if ent is not None and ent[1] == ver:
            _PACK_CACHE.move_to_end(key)
            _PACK_STATS["hit"] += 1
            return ent[2]
    pm = PackedMask.pack(m)
    _PACK_STATS["pack"] += 1
    with _WS_LOCK:
        _PACK_CACHE[key] = (m, ver, pm)
        _PACK_CACHE.move_to_end(key)
        while len(_PACK_CACHE) > _PACK_CACHE_MAX:
            _PACK_CACHE.popitem(last=False)
    return pm


def _compact_2d(geom, f_gp):
    """Does a 2-D call of this geometry and forcing take bit-packed masks / box faces (all conditions of that kind, constant values)?  What
    dn_poisson_query answers as `compact`, restated for the two places that must not make a foreign call: `_auto_pack` runs on every call
    before the cache key, `_fused` under torch.compile.  tests/test_poisson_query_host.py holds the two equal."""
    return geom.nsd == 2 and geom.deg == 1 and f_gp is None and not _lib.CONFIG_MIRROR.get("Q1_RULE_KERNEL")


def _auto_pack(geom, u, f_gp, dl):
    """The conditions of a one-shot 2-D Q1 call with their mask IMAGES replaced by (cached) bit-packed masks, where the compact kernels
    take the whole call: every condition a constant value on a PackedMask / BoxFaces / contiguous float32, uint8 or bool CUDA image."""
    if not (AUTO_PACK_MASKS and _compact_2d(geom, f_gp) and len(dl) > 0 and isinstance(u, torch.Tensor) and u.is_cuda):
        return dl
    want = (1, *geom.node_shape)
    for d in dl:
        m = d.mask
        if isinstance(d.value, torch.Tensor):
            return dl
        if isinstance(m, (PackedMask, BoxFaces)):
            continue
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.device == u.device and m.is_contiguous() and not m.requires_grad and
                m.dtype in (torch.float32, torch.uint8, torch.bool) and m.dim() == u.dim() and tuple(m.shape[1:]) == want and
                m.shape[0] in (1, u.shape[0])):
            return dl
    if any(isinstance(d.mask, torch.Tensor) and _version_of(d.mask) is None for d in dl):
        return dl
    return [d if isinstance(d.mask, (PackedMask, BoxFaces)) else Dirichlet(_packed_on_first_use(d.mask), d.value) for d in dl]


def _norm_dirichlet(dirichlet):
    out = []
    for d in dirichlet or ():
        if isinstance(d, Dirichlet):
            out.append(d)
        else:
            m, v = d
            out.append(Dirichlet(m, v))
    if len(out) > 2:
        raise ValueError("at most two Dirichlet conditions per call are supported; merge masks beforehand")
    return out


_threading = __import__("threading")
_WS_LOCK = _threading.Lock()


_SIDE_STREAMS = {}


def _side_stream(dev):
    """One side stream per device for the deferred final reductions (PoissonPlan(async_sums=True))."""
    s = _SIDE_STREAMS.get(dev.index)
    if s is None:
        s = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(dev)
    return s


def workspace_status(device=None):
    """Health check of the shared launch workspaces of `device` (every stream that has used one): synchronises those streams and raises
    DiffNetHipError if a launch ran a bounded LDS hand-over poll to its limit (chained-strip plans; such a launch's outputs and sums are
    NaN -- never silently wrong).  Cheap enough for once per epoch; not for the launch path."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with _WS_LOCK:
        items = [(k, w) for op in (_POISSON, _FSDT) for k, w in op.ws.items() if k[0] == dev.index]
    for (_, stream), ws in items:
        _lib.check(_lib.lib().dn_workspace_status(C.c_void_p(ws.data_ptr()), C.c_void_p(stream)), "dn_workspace_status")


# ---- one-shot calls: prepared launches cached behind the public API ------------------------------------------------------------
# energy_loss / energy_loss_and_grad / residual* evaluate the operator on the same buffers step after step (a training loop's network
# output lands in the same allocator block every iteration).  Validation and the argument structs of such a call are kept in a small
# LRU keyed on everything they depend on -- pointers, shapes, condition forms, coefficients, stream -- so that a repeat costs the key,
# the output allocations and one ctypes call instead of the full preparation (22 -> ~8 us of host time: small meshes are bounded by
# the device, not by Python).  An entry holds NO reference to the caller's tensors (a pointer + shape is all a launch needs, and the
# caller passes live tensors to every call); outputs are allocated fresh per call (a cached call never overwrites an earlier result).
# Every operator has a cache of its own (_FusedOp.cache below; the Poisson one is _POISSON.cache), bounded by _CALL_CACHE_MAX.
_CALL_CACHE_MAX = 16
_CALL_STATS = {"hit": 0, "miss": 0, "uncached": 0}


def _tkey(t):
    """What a launch depends on for a tensor argument that is used as it is; None when it would need a conversion copy."""
    if t is None:
        return 0
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
        return None
    return (t.data_ptr(), t.dtype, tuple(t.shape))


def _call_key(geom, u, nu, f, f_gp, dl, scal, want_out, want_sums, out):
    parts = [geom.key, u.device.index, _raw_stream(u.device), scal, want_out, want_sums, isinstance(f, LoadVector)]
    if isinstance(f, LoadVector):
        f = f.tensor
    for t in (u, nu, f, f_gp, out):
        k = _tkey(t)
        if k is None or (k != 0 and k[1] != torch.float32):
            return None
        parts.append(k)
    for d in dl:
        m, v = d.mask, d.value
        if isinstance(m, PackedMask):
            mk = ("bits", m.bits.data_ptr(), m.shape)
        elif isinstance(m, BoxFaces):
            mk = ("box", m.bits)
        else:
            mk = _tkey(m)
            if mk is None or mk == 0 or mk[1] not in (torch.float32, torch.uint8):
                return None
        if isinstance(v, torch.Tensor):
            vk = _tkey(v)
            if vk is None or vk[1] != torch.float32 or len(vk[2]) != u.dim():
                return None
        else:
            vk = float(v)
        parts.append((mk, vk))
    return tuple(parts)


def poisson_apply(geom, u, nu=None, f=None, f_gp=None, dirichlet=(), alpha=1.0, beta=1.0, c=1.0, wscale=1.0,
                  out_scale=1.0, want_out=True, want_sums=True, loss_scale=None, out=None):
    """One launch of dn_poisson_apply.  Returns (out | None, sums | None) where sums is a float64 device
    tensor [energy, sum(out_unscaled^2)].  With `loss_scale` a third value is returned: the 0-dim float32 tensor
    energy * loss_scale written by the same launch.  See include/diffnet_hip.h for the operator definition."""
    dl = _auto_pack(geom, u, f_gp, _norm_dirichlet(dirichlet))
    key = None
    if isinstance(u, torch.Tensor) and u.is_cuda:
        key = _call_key(geom, u, nu, f, f_gp, dl, (float(alpha), float(beta), float(c), float(wscale), float(out_scale),
                                                   None if loss_scale is None else float(loss_scale)), want_out, want_sums, out)
    if key is None:            # something needs a conversion copy (or is invalid: the full preparation says what)
        _CALL_STATS["uncached"] += 1
        return PoissonPlan(geom, u, nu, f, f_gp, dl, alpha, beta, c, wscale, out_scale, want_out, want_sums, loss_scale, out, strict=False).launch()
    cache = _POISSON.cache
    with _WS_LOCK:
        ent = cache.get(key)
        if ent is not None:
            cache.move_to_end(key)
    if ent is None:
        _CALL_STATS["miss"] += 1
        plan = PoissonPlan(geom, u, nu, f, f_gp, dl, alpha, beta, c, wscale, out_scale, want_out, want_sums, loss_scale, out, strict=True)
        res = plan.launch()
        # keep the structs, the workspace and the condition objects' own cached images; drop the caller's tensors and this call's outputs
        with _WS_LOCK:
            live_ws = list(_POISSON.ws.values())
        plan.keep = [t for t in plan.keep if any(t is w for w in live_ws)] + [d.mask for d in dl if not isinstance(d.mask, torch.Tensor)]
        plan.result = None
        plan.fresh = (want_out and out is None, want_sums, loss_scale is not None)
        with _WS_LOCK:
            cache[key] = plan
            while len(cache) > _CALL_CACHE_MAX:
                cache.popitem(last=False)
        return res
    _CALL_STATS["hit"] += 1
    a = ent.args
    new_out, has_sums, has_loss = ent.fresh
    o = out
    sums = loss32 = None
    if new_out:
        o = torch.empty_like(u)
    if has_sums:
        sums = torch.empty(2, dtype=torch.float64, device=u.device)
    if has_loss:
        loss32 = torch.empty((), dtype=torch.float32, device=u.device)
    # the entry's argument struct is shared by every caller that hits this key: the output pointers are patched and the launch is issued
    # under the entry's lock, so two Python threads on the same (stream, buffers) cannot interleave them
    with ent.lock:
        if new_out:
            a.out = o.data_ptr()
        if has_sums:
            a.energy = sums.data_ptr()
            a.sumsq = a.energy + 8
        if has_loss:
            a.energy_f32 = loss32.data_ptr()
        rc = ent._fn(ent._mesh_ref, ent._args_ref, C.c_void_p(key[2]))
    if rc:
        _lib.check(rc, "dn_poisson_apply")
    return (o, sums, loss32) if has_loss else (o, sums)


def call_cache_clear():
    """Forget the cached prepared calls (after dn_config_set of a launch-plan switch: the workspace size depends on the plan)."""
    with _WS_LOCK:
        for op in _FUSED_OPS:
            op.cache.clear()
            op.ws_bytes.clear()
        _PACK_CACHE.clear()


class PoissonPlan:
    """A dn_poisson_apply call prepared once for FIXED buffers: validation, the argument structs, the outputs and the workspace are
    set up at construction; `launch()` is one ctypes call (~3 us of host time instead of ~25).  For loops that evaluate the operator
    on the same tensors every step -- the slab-parallel path (diffnet_amd/slab.py), whose per-rank kernels are shorter than the
    host-side preparation -- and for anything captured into a HIP graph.  Outputs are overwritten by every launch."""

    def __init__(self, geom, u, nu=None, f=None, f_gp=None, dirichlet=(), alpha=1.0, beta=1.0, c=1.0, wscale=1.0,
                 out_scale=1.0, want_out=True, want_sums=True, loss_scale=None, out=None, strict=True, strip_select=0, continues=None,
                 async_sums=False, loss_out=None, pipelined_sums=False):
        """pipelined_sums (round 4): the launch leaves per-workgroup partial sums in a workspace of its own and does NOT form its scalars; the
        NEXT launch in the loop does, at its start (`nxt.fold(this)`: dn_poisson_args.fold_prev -- the first workgroup of that launch adds the
        partials up before its own march), and `finish_sums()` closes the last evaluation of a loop with the one-workgroup kernel.  The
        final reduction (a ~3 us serial tail of a ~56 us launch: every workgroup has finished, the last arriver adds 2048 partials) leaves the
        critical path without a side stream or an event; the price: the loss of step k is ready when launch k + 1 has run (a training loop
        only logs it).  The gradient is final when its own launch ends, as always.
        async_sums: the launch leaves per-workgroup partial sums; the final scalars are formed by a one-workgroup kernel on a SIDE stream
        (dn_poisson_finish_sums), i.e. under whatever the launch stream runs next -- the in-kernel final reduction is a ~3 us serial tail
        of every launch.  The gradient is ready in launch-stream order as always; the sums / the loss are ready on the side stream: call
        `wait_sums()` (makes the current stream wait for them) before consuming them there, or consume them under `sums_stream`.  Such a
        plan owns its reduction workspace.
        strip_select 1 / 2: the launch covers only the first + last strip of the marched axis / all the others (include/diffnet_hip.h:
        split evaluation); `continues`: the PoissonPlan of the first launch of such a pair -- this one writes into its outputs and adds
        its sums to that launch's."""
        # strict: every tensor argument must be usable as it is (contiguous float32 fields, float32 / uint8 mask images) -- a conversion
        # would be a one-time copy that later launches keep reading after the caller has updated the original in place
        if continues is not None:
            out = continues.result[0]
        self.mesh, self.args, self.keep, self.result = _prepare_poisson(geom, u, nu, f, f_gp, dirichlet, alpha, beta, c, wscale, out_scale,
                                                                        want_out, want_sums, loss_scale, out, strict=strict,
                                                                        reuse=None if continues is None else continues.result)
        if loss_out is not None:
            # the float32 loss goes into the caller's one-element tensor (e.g. a slot of a buffer that one collective reduces for several steps)
            if loss_scale is None or continues is not None:
                raise ValueError("loss_out needs loss_scale and is not for the second launch of a split evaluation")
            if not (isinstance(loss_out, torch.Tensor) and loss_out.is_cuda and loss_out.dtype == torch.float32 and loss_out.numel() == 1
                    and loss_out.device == u.device):
                raise DiffNetHipError("loss_out must be a one-element float32 tensor on the device of u")
            self.args.energy_f32 = loss_out.data_ptr()
            self.keep.append(loss_out)
            self.result = (self.result[0], self.result[1], loss_out)
        self.args.strip_select = int(strip_select)
        self.args.accumulate_sums = int(continues is not None)
        self.async_sums = bool(async_sums) and self.args.workspace is not None and self.args.workspace != 0
        self.pipelined_sums = bool(pipelined_sums) and not self.async_sums and self.args.workspace is not None and self.args.workspace != 0
        self._folds = None
        if self.pipelined_sums:
            self.args.defer_sums = 1
            ws = torch.zeros(int(self.args.workspace_bytes), dtype=torch.uint8, device=u.device)      # its own: the partials wait for the next launch
            self.keep.append(ws)
            self.args.workspace = ws.data_ptr()
        if self.async_sums:
            self.args.defer_sums = 1
            ws = torch.zeros(int(self.args.workspace_bytes), dtype=torch.uint8, device=u.device)      # its own: the partials wait for the side stream
            self.keep.append(ws)
            self._own_ws = ws
            self.args.workspace = ws.data_ptr()
            self.sums_stream = _side_stream(u.device)
            self._side = self.sums_stream.cuda_stream
            self._ev_main, self._ev_done = _lib.new_event(), _lib.new_event()
            self._hip = _lib.hip_runtime()
            self._finish = _lib.lib().dn_poisson_finish_sums
            self._launched = False
        self.device = u.device
        self.stream = _raw_stream(u.device)      # the reduction workspace belongs to this stream
        self._fn = _lib.lib().dn_poisson_apply
        self._mesh_ref, self._args_ref = C.byref(self.mesh), C.byref(self.args)
        self.lock = _threading.Lock()            # guards the shared argument struct of a cached call (ops.poisson_apply)
        if self.async_sums:
            # the partials, the sums and the loss are allocated on the launch stream but read / written by the finish kernel on the side
            # stream: tell the caching allocator, or a dropped plan's blocks could be handed to launch-stream work while that kernel is pending
            for t in [self._own_ws] + [r for r in self.result[1:] if isinstance(r, torch.Tensor)]:
                t.record_stream(self.sums_stream)

    def __del__(self):
        if getattr(self, "async_sums", False):
            try:
                hip = self._hip
                if getattr(self, "_launched", False):
                    hip.hipEventSynchronize(self._ev_done)       # the finish kernel still reads the plan's workspace
                hip.hipEventDestroy(self._ev_main)
                hip.hipEventDestroy(self._ev_done)
            except Exception:                                     # interpreter shutdown: the runtime may already be gone
                pass

    def check(self):
        """Health check of the plan's workspace (synchronises the stream): raises if a launch that used it ran a bounded hand-over poll
        to its limit (its results are NaN then; include/diffnet_hip.h: dn_workspace_status)."""
        if self.args.workspace:
            _lib.check(_lib.lib().dn_workspace_status(C.c_void_p(self.args.workspace), C.c_void_p(_raw_stream(self.device))), "dn_workspace_status")

    def launch(self):
        cur = _raw_stream(self.device)
        if self.args.workspace and cur != self.stream:
            raise DiffNetHipError("PoissonPlan.launch: prepared on another stream (its reduction workspace is per stream); prepare one plan per stream")
        if self.async_sums:
            hip, side = self._hip, C.c_void_p(self._side)
            if self._launched:
                hip.hipStreamWaitEvent(C.c_void_p(cur), self._ev_done, 0)      # the previous evaluation's partials and scalars have been consumed
            rc = self._fn(self._mesh_ref, self._args_ref, C.c_void_p(cur))
            if rc:
                _lib.check(rc, "dn_poisson_apply")
            hip.hipEventRecord(self._ev_main, C.c_void_p(cur))
            hip.hipStreamWaitEvent(side, self._ev_main, 0)
            rc = self._finish(self._mesh_ref, self._args_ref, side)
            if rc:
                _lib.check(rc, "dn_poisson_finish_sums")
            hip.hipEventRecord(self._ev_done, side)
            self._launched = True
            return self.result
        rc = self._fn(self._mesh_ref, self._args_ref, C.c_void_p(cur))
        if rc:
            _lib.check(rc, "dn_poisson_apply")
        return self.result

    def fold(self, prev):
        """This launch closes the evaluation of `prev` (a pipelined_sums plan on the same mesh and batch, prepared on the same stream, whose launch
        precedes this one there): its first workgroup adds up prev's partial sums and writes prev's scalars (a split launch left without strips
        runs the one-workgroup finish kernel for that).  Raises DiffNetHipError for a plan of another mesh, batch, device or stream.
        fold(None) clears."""
        if prev is None:
            self.args.fold_prev = None
            self._folds = None
            return self
        if not getattr(prev, "pipelined_sums", False):
            raise DiffNetHipError("PoissonPlan.fold: the other plan must be prepared with pipelined_sums=True")
        # the library counts prev's partial sums and finds their stride from THIS launch's mesh struct (batch included): they must be identical
        if C.string_at(C.addressof(prev.mesh), C.sizeof(prev.mesh)) != C.string_at(C.addressof(self.mesh), C.sizeof(self.mesh)):
            raise DiffNetHipError("PoissonPlan.fold: the other plan was prepared for another mesh or batch size; only a plan on the same mesh "
                                  "and batch can be folded")
        if prev.device != self.device or prev.stream != self.stream:
            raise DiffNetHipError("PoissonPlan.fold: the other plan was prepared on another device or stream; its launch must precede this one "
                                  "on the same stream")
        self._folds = prev                                    # keeps its argument struct and workspace alive
        self.args.fold_prev = C.addressof(prev.args)
        return self

    def finish_sums(self):
        """pipelined_sums: form this plan's scalars from the partial sums of its last launch now (one small kernel on the current stream)
        -- for the last evaluation of a loop, which no further launch folds."""
        if not self.pipelined_sums:
            return self.result
        rc = _lib.lib().dn_poisson_finish_sums(self._mesh_ref, self._args_ref, C.c_void_p(_raw_stream(self.device)))
        if rc:
            _lib.check(rc, "dn_poisson_finish_sums")
        return self.result

    def wait_sums(self):
        """async_sums: make the current stream wait for the sums / the loss of the last launch (no-op otherwise)."""
        if self.async_sums and self._launched:
            self._hip.hipStreamWaitEvent(C.c_void_p(_raw_stream(self.device)), self._ev_done, 0)


def _dirichlet_image(bc, m, value, u, node_shape, keep, strict=False):
    """One Dirichlet condition read as a mask image into the dn_dirichlet `bc` of a call on u (B,1,*node_shape): the mask `m` (any form) as
    a contiguous float32 / uint8 image, the value as a constant or a nodal field.  Returns the image.  `strict` (PoissonPlan): a mask or a
    value field that would need a conversion copy is refused."""
    nsd, B = len(node_shape), u.shape[0]
    m = _mask_image(m, u)
    if not isinstance(m, torch.Tensor) or not m.is_cuda:
        raise DiffNetHipError("Dirichlet mask must be a CUDA tensor")
    if strict and (m.dtype == torch.bool or not m.is_contiguous()):
        raise DiffNetHipError("PoissonPlan: a bool or non-contiguous Dirichlet mask would be converted into a one-time copy; pass a "
                              "contiguous float32 / uint8 image (or a PackedMask / BoxFaces)")
    if m.dtype == torch.bool:
        m = m.to(torch.uint8)
    if m.dtype not in (torch.float32, torch.uint8):
        raise TypeError("Dirichlet mask must be float32, uint8 or bool")
    m = m.contiguous()
    if m.dim() != nsd + 2 or tuple(m.shape[1:]) != (1, *node_shape) or m.shape[0] not in (1, B):
        raise ValueError(f"Dirichlet mask shape {tuple(m.shape)} does not match u")
    keep.append(m)
    bc.mask = m.data_ptr()
    bc.mask_kind = _lib.MASK_U8 if m.dtype == torch.uint8 else _lib.MASK_F32
    bc.mask_batched = int(m.shape[0] == B)
    if isinstance(value, torch.Tensor):
        v = value
        if v.dim() == nsd:
            v = v[(None,) * 2]
        if strict and not v.is_cuda:
            raise DiffNetHipError("PoissonPlan: the Dirichlet value field must live on the GPU (a prepared launch would keep a one-time copy)")
        v = _require(v.to(u.device) if not v.is_cuda else v, "Dirichlet value", nsd + 2, strict)
        if tuple(v.shape[1:]) != (1, *node_shape) or v.shape[0] not in (1, B):
            raise ValueError("Dirichlet value field shape does not match u")
        keep.append(v)
        bc.field = v.data_ptr()
        bc.field_batched = int(v.shape[0] == B)
    else:
        bc.value = float(value)
    return m


def _prepare_poisson(geom, u, nu, f, f_gp, dirichlet, alpha, beta, c, wscale, out_scale, want_out, want_sums, loss_scale, out, strict=False, reuse=None):
    """Validation + argument structs of one dn_poisson_apply call: (mesh, args, tensors to keep alive, result tuple)."""
    nsd = geom.nsd
    u = _require(u, "u", nsd + 2, strict)
    B = u.shape[0]
    node_shape = tuple(geom.node_shape)            # (ny, nx) or (nz, ny, nx)
    if tuple(u.shape[1:]) != (1, *node_shape):
        raise ValueError(f"u has shape {tuple(u.shape)}, expected (B,1,{','.join(map(str, node_shape))})")
    keep = [u]
    args = DnPoissonArgs()
    args.u = u.data_ptr()

    def field(t, name, allow_gp=False):
        t = _require(t, name, nsd + 2, strict)
        if t.shape[0] not in (1, B):
            raise ValueError(f"{name} batch {t.shape[0]} does not broadcast to {B}")
        keep.append(t)
        return t, int(t.shape[0] == B)

    if nu is not None:
        nu, nb_ = field(nu, "nu")
        if tuple(nu.shape[1:]) != (1, *node_shape):
            raise ValueError("nu must be a nodal field")
        args.nu, args.nu_batched = nu.data_ptr(), nb_
    if f is not None and f_gp is not None:
        raise ValueError("give either nodal f or f_gp, not both")
    if isinstance(f, LoadVector):
        args.f_is_load = 1
        f = f.tensor
    if f is not None:
        f, fb = field(f, "f")
        if tuple(f.shape[1:]) != (1, *node_shape):
            raise ValueError("f must be a nodal field")
        args.f, args.f_batched = f.data_ptr(), fb
    if f_gp is not None:
        f_gp, fb = field(f_gp, "f_gp")
        if tuple(f_gp.shape[1:]) != (geom.ngp_total, *geom.elem_shape):
            raise ValueError(f"f_gp must have shape (B|1,{geom.ngp_total},{geom.elem_shape})")
        args.f_gp, args.f_batched = f_gp.data_ptr(), fb
    dl = _norm_dirichlet(dirichlet)
    args.alpha, args.beta, args.c, args.wscale, args.out_scale = alpha, beta, c, wscale, out_scale
    mesh = geom.mesh_struct(B)
    if out is not None:
        if not want_out or out.shape != u.shape or out.dtype != torch.float32 or out.device != u.device or not out.is_contiguous():
            raise ValueError("out= must be a contiguous float32 tensor of u's shape on u's device")
    elif want_out:
        out = torch.empty_like(u)
    sums = None
    if out is not None:
        args.out = out.data_ptr()
    if want_sums or (mesh.nsd == 3 and mesh.degree > 1):       # (3-D Q2 / Q3: the workspace also holds the element vectors)
        ws = _op_workspace(_POISSON, mesh, B, u.device)
        keep.append(ws)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    if want_sums:
        sums = reuse[1] if reuse is not None else torch.empty(2, dtype=torch.float64, device=u.device)
        args.energy = sums.data_ptr()
        args.sumsq = sums.data_ptr() + 8
    loss32 = None
    if loss_scale is not None:
        if not want_sums:
            raise ValueError("loss_scale needs want_sums=True")
        loss32 = reuse[2] if reuse is not None else torch.empty((), dtype=torch.float32, device=u.device)
        args.energy_f32, args.energy_scale = loss32.data_ptr(), float(loss_scale)

    # Conditions last: every other pointer of the call is in `args` by now.  PackedMask / BoxFaces conditions with a constant value go in
    # as they are (bit arrays / box faces: no image is read) and the library is asked whether the launch of exactly these arguments takes them
    # (dn_poisson_query: the 2-D closed-form Q1 kernel takes both kinds, the 3-D two-element kernels box faces beside at most one image);
    # where it answers DN_E_UNSUPPORTED they are expanded to their (cached) uint8 images.
    def conditions(compact):
        for k, d in enumerate(dl):
            m, bc = d.mask, args.bc[k]
            if not (compact and isinstance(m, (PackedMask, BoxFaces)) and not isinstance(d.value, torch.Tensor)):
                _dirichlet_image(bc, m, d.value, u, node_shape, keep, strict)
                continue
            bc.value = float(d.value)
            if isinstance(m, BoxFaces):
                bc.mask_kind, bc.box_faces = _lib.MASK_BOX, m.bits
            else:
                if tuple(m.shape[1:]) != (1, *node_shape) or m.shape[0] not in (1, B) or m.bits.device != u.device:
                    raise ValueError(f"packed Dirichlet mask of shape {m.shape} does not match u")
                keep.append(m.bits)
                bc.mask, bc.mask_kind, bc.row_words = m.bits.data_ptr(), _lib.MASK_BITS, m.row_words
                bc.mask_batched = int(m.shape[0] == B)

    compact = any(isinstance(d.mask, (PackedMask, BoxFaces)) and not isinstance(d.value, torch.Tensor) for d in dl)
    if compact:
        nkeep = len(keep)
        conditions(True)
        if _lib.lib().dn_poisson_query(C.byref(mesh), C.byref(args), C.byref(_lib.DnPoissonKernel())) == -2:      # DN_E_UNSUPPORTED
            del keep[nkeep:]
            for k in range(2):
                args.bc[k] = _lib.DnDirichlet()
            compact = False
    if not compact:
        conditions(False)
    keep += [t for t in (out, sums, loss32) if t is not None]
    return mesh, args, keep, ((out, sums, loss32) if loss_scale is not None else (out, sums))


# ---- composed (operator-level) forms: differentiable wrt EVERY tensor input ------------------------------------
# The fused kernels return the gradient wrt u only.  When a coefficient (nu, f, f_gp) or a Dirichlet value field requires a
# gradient -- inverse / parametric-coefficient problems, which the reference differentiates through plain autograd
# (IBN_2D.py:116-134) -- the same loss is evaluated on the single-launch HIP operators (`_GaussPtEval` and its adjoint) plus
# torch elementwise ops, so autograd covers all of them.  Slower (Gauss-point tensors are materialised), never silently wrong.
def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _extra_grad_inputs(nu, f, f_gp, dirichlet):
    return _wants_grad(nu, f, f_gp, *[d.value for d in dirichlet])


def _dirichlet_cond(m):
    return (m > 0.5) if m.is_floating_point() else (m != 0)


def _apply_dirichlet(u, dirichlet):
    for d in dirichlet:
        v = d.value
        if isinstance(v, torch.Tensor):
            v = v[(None,) * (u.dim() - v.dim())] if v.dim() < u.dim() else v
            v = v.to(u.device).expand_as(u)
        else:
            v = torch.full_like(u, float(v))
        u = torch.where(_dirichlet_cond(_mask_image(d.mask, u)), v, u)
    return u


def _geom_tables(geom, device):
    """Stacked (G, nbf^nsd) N / dN_d tables and the nd weights of a FemGeometry on `device` (cached)."""
    cache = geom.__dict__.setdefault("_dev_tables", {})
    hit = cache.get(str(device))
    if hit is None:
        from .tables import nd_tables
        K, _, w = nd_tables(geom.nsd, geom.deg, geom.gpx_1d, geom.gpw_1d, geom.hs)
        names = ["N_gp"] + ["dN_%s_gp" % a for a in "xyz"[:geom.nsd]]
        hit = ({n: torch.from_numpy(K[n].reshape(K[n].shape[0], -1).copy()).to(device) for n in names}, torch.from_numpy(w).to(device))
        cache[str(device)] = hit
    return hit


def composed_energy(geom, u, nu=None, f=None, f_gp=None, dirichlet=(), c=1.0, jac=1.0):
    """Energy loss on the drop-in operators (the reference formulation, e.g. IBN_2D.py:116-134): differentiable wrt u, nu, f,
    f_gp and Dirichlet value fields."""
    T, w = _geom_tables(geom, u.device)
    nsd, nbf = geom.nsd, geom.deg + 1
    ev = lambda t, name: _GaussPtEval.apply(t, T[name], nsd, nbf, nbf - 1)
    ub = _apply_dirichlet(u, _norm_dirichlet(dirichlet))
    g2 = sum(ev(ub, "dN_%s_gp" % a) ** 2 for a in "xyz"[:nsd])
    wg = (w * jac).reshape((1, -1) + (1,) * nsd)
    dens = c * g2 if nu is None else c * ev(nu, "N_gp") * g2
    if f is not None or f_gp is not None:
        dens = dens - ev(ub, "N_gp") * (f_gp if f_gp is not None else ev(f, "N_gp"))
    return torch.sum(wg * dens) / (u.shape[0] * geom.nelem_total)


def composed_residual(geom, u, nu=None, f=None, f_gp=None, dirichlet=(), jac=1.0):
    """Assembled weak-form residual (zero on Dirichlet nodes) from the operator adjoints: R = sum_d gpe^T(W nu d_d u ; dN_d)
    - gpe^T(W f ; N).  Differentiable wrt every tensor input."""
    T, w = _geom_tables(geom, u.device)
    nsd, nbf = geom.nsd, geom.deg + 1
    dirichlet = _norm_dirichlet(dirichlet)
    ev = lambda t, name: _GaussPtEval.apply(t, T[name], nsd, nbf, nbf - 1)
    evT = lambda t, name: _GaussPtEvalT.apply(t.contiguous(), T[name], tuple(u.shape), nsd, nbf, nbf - 1)
    ub = _apply_dirichlet(u, dirichlet)
    wg = (w * jac).reshape((1, -1) + (1,) * nsd)
    nug = None if nu is None else ev(nu, "N_gp")
    R = None
    for a in "xyz"[:nsd]:
        q = wg * ev(ub, "dN_%s_gp" % a)
        q = q if nug is None else q * nug
        t = evT(q.expand(u.shape[0], *q.shape[1:]), "dN_%s_gp" % a)
        R = t if R is None else R + t
    if f is not None or f_gp is not None:
        fg = f_gp if f_gp is not None else ev(f, "N_gp")
        R = R - evT((wg * fg).expand(u.shape[0], -1, *fg.shape[2:]), "N_gp")
    for d in dirichlet:
        R = torch.where(_dirichlet_cond(_mask_image(d.mask, R)), torch.zeros_like(R), R)
    return R


class _PoissonFn(torch.autograd.Function):
    """(out, sums, loss) of one dn_poisson_apply launch, differentiable wrt u -- the eager counterpart of the registered operator
    diffnet_mi::poisson_apply (torch_ops.py), whose dispatch costs ~100 us per call (204 -> ~60 us for an energy_loss + backward at
    64^2, tools/host_profile.py); same formulas as torch_ops._pa_backward, and differentiable again (its backward calls `_fused`).
    Also differentiable wrt nu and the nodal f: the operator is bilinear in ((nu, f), u~), and the transpose of u~ -> out with respect to
    (nu, f) is one dn_poisson_coef_grad launch (`_coef`) per cotangent that arrives."""

    @staticmethod
    def forward(ctx, u, nu, f, f_gp, geom, dl, alpha, beta, c, wscale, out_scale, loss_scale):
        out, sums, loss = poisson_apply(geom, u, nu, f, f_gp, dl, alpha=alpha, beta=beta, c=c, wscale=wscale, out_scale=out_scale,
                                        want_out=True, want_sums=True, loss_scale=loss_scale)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(out, nu, u)
        ctx.meta = (geom, dl, alpha, beta, c, wscale, out_scale, loss_scale)
        ctx.f_shape = tuple(f.shape) if isinstance(f, torch.Tensor) else None
        return out, sums, loss

    @staticmethod
    def backward(ctx, g_out, g_sums, g_loss):
        out, nu, u = ctx.saved_tensors
        geom, dl, alpha, beta, c, wscale, out_scale, loss_scale = ctx.meta
        need_u, need_nu, need_f = ctx.needs_input_grad[:3]
        gnu = gf = None

        def coef_add(v, a_nu, a_f, in_scale=None):
            nonlocal gnu, gf
            tn, tf = _coef(geom, u, v, dl, a_nu, a_f, wscale, need_nu, need_f, in_scale)
            if tn is not None:
                gnu = tn if gnu is None else gnu + tn
            if tf is not None:
                gf = tf if gf is None else gf + tf

        if need_nu or need_f:
            # out = out_scale Z (alpha K_nu u~ - beta F f);  sumsq = sum (out / out_scale)^2;  energy = sum W (c nu |grad u~|^2 - u~ f)
            if g_out is not None:
                coef_add(g_out.contiguous(), out_scale * alpha, -out_scale * beta)
            if g_sums is not None:
                coef_add(out * (2.0 / out_scale), alpha, -beta, g_sums[1:2].to(torch.float32))
        hom = tuple(Dirichlet(d.mask, 0.0) for d in dl)       # J = s alpha M K M is symmetric: J^T v is the same launch, homogeneous conditions, no forcing

        def K(v, scale):
            return _fused(geom, v, nu, None, None, hom, alpha, 0.0, 0.0, wscale, scale, 0.0)[0]

        gu = None
        if g_out is not None and need_u:
            gu = K(g_out.contiguous(), out_scale)
        coef = None
        if g_loss is not None:
            coef = g_loss * loss_scale
        if g_sums is not None:
            coef = g_sums[0].to(torch.float32) if coef is None else coef + g_sums[0].to(torch.float32)
            if need_u:
                t = K(out * (2.0 / out_scale), 1.0) * g_sums[1].to(torch.float32)
                gu = t if gu is None else gu + t
        if coef is not None:
            if alpha != 2.0 * c or beta != 1.0:
                if g_loss is not None or c != 0.0:
                    raise RuntimeError("poisson_apply: the energy output is differentiable only in the energy-loss form (alpha = 2c, beta = 1)")
            else:
                t = out * (coef / out_scale)
                gu = t if gu is None else gu + t
                if need_nu or need_f:
                    coef_add(None, c, -1.0, coef.reshape(1))
        if gnu is not None and nu.shape[0] != gnu.shape[0]:
            gnu = gnu.sum(0, keepdim=True)               # one coefficient shared by the batch
        if gf is not None and ctx.f_shape[0] != gf.shape[0]:
            gf = gf.sum(0, keepdim=True)
        return (gu if need_u else None, gnu, gf) + (None,) * 9


def _fused(geom, u, nu, f, f_gp, dirichlet, alpha, beta, c, wscale, out_scale, loss_scale):
    """(out, sums, loss) of one dn_poisson_apply launch, differentiable wrt u through all three outputs.  Under torch.compile /
    torch.export the registered operator diffnet_mi::poisson_apply (an ordinary graph node); in eager mode the same launch behind a
    plain autograd.Function, or directly when nothing requires a gradient."""
    if torch.compiler.is_compiling():
        from . import torch_ops
        if isinstance(f, LoadVector):
            raise DiffNetHipError("LoadVector forcing is an eager-mode argument (the registered operator takes tensors); pass nodal f under torch.compile")
        compact = _compact_2d(geom, f_gp) and all(not isinstance(d.value, torch.Tensor) for d in dirichlet)
        return torch_ops.poisson_apply(u, nu, f, f_gp, *torch_ops.dirichlet_args(dirichlet, u, compact), *torch_ops.geometry_args(geom),
                                       float(alpha), float(beta), float(c), float(wscale), float(out_scale), float(loss_scale))
    for d in dirichlet:
        if isinstance(d.mask, torch.Tensor) and d.mask.dtype == torch.int32:
            raise TypeError("Dirichlet mask images are float32, uint8 or bool; int32 tensors are reserved for bit-packed masks (wrap them in ops.PackedMask)")
    if _wants_grad(u, nu, None if isinstance(f, LoadVector) else f):
        return _PoissonFn.apply(u, nu, f, f_gp, geom, tuple(dirichlet), float(alpha), float(beta), float(c), float(wscale), float(out_scale),
                                float(loss_scale))
    return poisson_apply(geom, u, nu, f, f_gp, dirichlet, alpha=alpha, beta=beta, c=c, wscale=wscale, out_scale=out_scale, want_out=True,
                         want_sums=True, loss_scale=loss_scale)


def energy_loss(geom, u, nu=None, f=None, f_gp=None, dirichlet=(), c=1.0, jac=1.0):
    """mean_{b,e} sum_g gpw_g*jac*(c*nu_g*|grad u|_g^2 - u_g*f_g).  One fused launch, differentiable wrt u, and on Q1 meshes wrt nu and
    the nodal f (one dn_poisson_coef_grad launch in the backward pass); when f_gp or a Dirichlet value field requires a gradient, or on
    Q2 / Q3 meshes, the composed operator form runs instead (see composed_energy)."""
    dirichlet = tuple(_norm_dirichlet(dirichlet))
    if _extra_grad_inputs(nu, f, f_gp, dirichlet) and not _coef_route(geom, u, f_gp, dirichlet):
        return composed_energy(geom, u, nu, f, f_gp, dirichlet, float(c), float(jac))
    scale = 1.0 / (u.shape[0] * geom.nelem_total)
    return _fused(geom, u, nu, f, f_gp, dirichlet, 2.0 * c, 1.0, c, jac, scale, scale)[2]


def energy_loss_and_grad(geom, u, nu=None, f=None, f_gp=None, dirichlet=(), c=1.0, jac=1.0, out=None):
    """(loss, dloss/du) from ONE kernel pass, outside autograd -- the form an optimiser loop wants and the
    form bench.py measures (16 algorithmic bytes per node: read u, nu, f; write grad).  `out`: optional preallocated
    gradient buffer (same shape as u)."""
    B = u.shape[0]
    scale = 1.0 / (B * geom.nelem_total)
    grad, _, loss = poisson_apply(geom, u.detach(), nu, f, f_gp, dirichlet, alpha=2.0 * c, beta=1.0, c=c, wscale=jac,
                                  out_scale=scale, want_out=True, want_sums=True, loss_scale=scale, out=out)
    return loss, grad


def residual(geom, u, nu=None, f=None, f_gp=None, dirichlet=(), jac=1.0):
    dirichlet = tuple(_norm_dirichlet(dirichlet))
    if _extra_grad_inputs(nu, f, f_gp, dirichlet) and not _coef_route(geom, u, f_gp, dirichlet):
        return composed_residual(geom, u, nu, f, f_gp, dirichlet, float(jac))
    return _fused(geom, u, nu, f, f_gp, dirichlet, 1.0, 1.0, 0.0, jac, 1.0, 0.0)[0]


def residual_loss(geom, u, nu=None, f=None, f_gp=None, dirichlet=(), jac=1.0):
    dirichlet = tuple(_norm_dirichlet(dirichlet))
    if _extra_grad_inputs(nu, f, f_gp, dirichlet) and not _coef_route(geom, u, f_gp, dirichlet):
        return torch.sum(composed_residual(geom, u, nu, f, f_gp, dirichlet, float(jac)) ** 2)
    return _fused(geom, u, nu, f, f_gp, dirichlet, 1.0, 1.0, 0.0, jac, 1.0, 0.0)[1][1].to(torch.float32)


# ---- gradient wrt the coefficient and the forcing (dn_poisson_coef_grad) --------------------------------------------------------------
# The fused operator is bilinear in ((nu, f), u~).  Its transpose with respect to (nu, f) is again a per-element quadrature followed by
# element -> node assembly: one launch (csrc/poisson_coef_grad.hip), no workspace, no reduction -- it touches no operator's workspace and
# no deferred partial sums, so it may stand between any two launches of a chained pair.
_COEF_STATS = {"launch": 0}


def _coef_route(geom, u, f_gp, dirichlet):
    """Does the fused route differentiate this call wrt nu / f?  Q1 meshes with rules of 2 to 4 points, eager mode, no gradient asked for
    f_gp or a Dirichlet value field, and dn_config_set("COEF_GRAD", "composed") not set (the route of before, for A/B runs)."""
    if torch.compiler.is_compiling() or _lib.CONFIG_MIRROR.get("COEF_GRAD") == "composed":
        return False
    if geom.deg != 1 or not 2 <= geom.ngp_1d <= 4 or not (isinstance(u, torch.Tensor) and u.is_cuda):
        return False
    return not _wants_grad(f_gp, *[d.value for d in dirichlet])


def poisson_coef_grad(geom, u, v=None, dirichlet=(), a_nu=1.0, a_f=1.0, wscale=1.0, want=("nu", "f"), in_scale=None):
    """One launch of dn_poisson_coef_grad (include/diffnet_hip.h): (g_nu | None, g_f | None), fresh (B,1,*N) tensors,
        g_nu[a] = a_nu s sum_e sum_g W_g N_a grad v_g . grad u~_g,    g_f[a] = a_f s sum_e sum_g W_g N_a v_g,    W_g = gpw_g wscale
    with u~ = u after the Dirichlet conditions, v read as zero on every Dirichlet node (v=None: v = u~) and s = in_scale[0] (a one-element
    float32 device tensor) or 1.  Outside autograd; Q1 meshes only.  PackedMask / BoxFaces conditions are expanded to their images."""
    nsd = geom.nsd
    u = _require(u, "u", nsd + 2)
    B = u.shape[0]
    node_shape = tuple(geom.node_shape)
    if tuple(u.shape[1:]) != (1, *node_shape):
        raise ValueError(f"u has shape {tuple(u.shape)}, expected (B,1,{','.join(map(str, node_shape))})")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ("nu", "f") for w in want):
        raise ValueError('want must name "nu" and / or "f"')
    keep = [u]
    args = DnCoefGradArgs()
    args.u = u.data_ptr()
    if v is not None:
        v = _require(v, "v", nsd + 2)
        if v.shape != u.shape or v.device != u.device:
            raise ValueError("v must have u's shape and device")
        keep.append(v)
        args.v = v.data_ptr()
    dl = _norm_dirichlet(dirichlet)
    imgs = [_dirichlet_image(args.bc[k], d.mask, d.value.detach().to(u.device) if isinstance(d.value, torch.Tensor) else d.value, u,
                             node_shape, keep) for k, d in enumerate(dl)]
    if len(imgs) == 2 and imgs[0].dtype != imgs[1].dtype:       # the kernels read both images in one format
        k = 0 if imgs[0].dtype == torch.float32 else 1
        m = (imgs[k] > 0.5).to(torch.uint8)
        keep.append(m)
        args.bc[k].mask, args.bc[k].mask_kind = m.data_ptr(), _lib.MASK_U8
    args.a_nu, args.a_f, args.wscale = float(a_nu), float(a_f), float(wscale)
    if in_scale is not None:
        in_scale = _require(in_scale, "in_scale")
        if in_scale.numel() != 1 or in_scale.device != u.device:
            raise ValueError("in_scale must hold one float on u's device")
        keep.append(in_scale)
        args.in_scale = in_scale.data_ptr()
    g_nu = torch.empty_like(u) if "nu" in want else None
    g_f = torch.empty_like(u) if "f" in want else None
    args.g_nu = g_nu.data_ptr() if g_nu is not None else None
    args.g_f = g_f.data_ptr() if g_f is not None else None
    mesh = geom.mesh_struct(B)
    rc = _lib.lib().dn_poisson_coef_grad(C.byref(mesh), C.byref(args), _stream(u))
    if rc:
        _lib.check(rc, "dn_poisson_coef_grad")
    _COEF_STATS["launch"] += 1
    return g_nu, g_f


# ---- the vector side of the CG solve (dn_poisson_diag, dn_poisson_cg): raw wrappers; the host layer is diffnet_amd/solve.py -----------
def poisson_diag(geom, batch, nu=None, dirichlet=(), wscale=1.0, unit=False, out=None, device=None):
    """One launch of dn_poisson_diag (include/diffnet_hip.h): the inverse diagonal of K_nu as a (batch,1,*N) float32 tensor, 0 on the
    Dirichlet nodes and where the diagonal is 0; unit=True: 1 on the other nodes.  PackedMask / BoxFaces conditions are expanded to
    their images; the conditions' values are not read.  Outside autograd; Q1 meshes only."""
    nsd, node_shape = geom.nsd, tuple(geom.node_shape)
    if out is None:
        if device is None:
            device = nu.device if isinstance(nu, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((int(batch), 1, *node_shape), dtype=torch.float32, device=device)
    out = _require(out, "out", nsd + 2, True)
    if tuple(out.shape) != (int(batch), 1, *node_shape):
        raise ValueError(f"out has shape {tuple(out.shape)}, expected ({batch},1,{','.join(map(str, node_shape))})")
    keep = [out]
    args = DnPoissonDiagArgs()
    if nu is not None:
        nu = _require(nu.detach(), "nu", nsd + 2)
        if tuple(nu.shape[1:]) != (1, *node_shape) or nu.shape[0] not in (1, batch) or nu.device != out.device:
            raise ValueError("nu must be a nodal field (B|1,1,*N) on the output's device")
        keep.append(nu)
        args.nu, args.nu_batched = nu.data_ptr(), int(nu.shape[0] == batch)
    for k, d in enumerate(_norm_dirichlet(dirichlet)):
        _dirichlet_image(args.bc[k], d.mask, 0.0, out, node_shape, keep)
    args.wscale, args.unit, args.dinv = float(wscale), int(bool(unit)), out.data_ptr()
    mesh = geom.mesh_struct(int(batch))
    rc = _lib.lib().dn_poisson_diag(C.byref(mesh), C.byref(args), _stream(out))
    if rc:
        _lib.check(rc, "dn_poisson_diag")
    return out


CG_PHASES = {"init": _lib.CG_INIT, "dot": _lib.CG_DOT, "update": _lib.CG_UPDATE, "direction": _lib.CG_DIRECTION}
# one dn_cg_state as a numpy record (the device block is read back as bytes)
CG_STATE_DTYPE = [("rz", "<f8"), ("rr", "<f8"), ("rr0", "<f8"), ("pq", "<f8"), ("alpha", "<f4"), ("beta", "<f4"),
                  ("active", "<i4"), ("iterations", "<i4"), ("flags", "<i4"), ("reserved", "<i4", (3,))]


def poisson_cg_workspace(n, batch, device):
    """A zero-filled workspace for dn_poisson_cg launches on samples of n nodes (one per stream in use)."""
    nbytes = int(_lib.lib().dn_poisson_cg_workspace_bytes(int(n), int(batch)))
    if nbytes <= 0:
        raise DiffNetHipError("dn_poisson_cg_workspace_bytes: n or batch out of range")
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def poisson_cg_state(batch, device):
    """A zeroed block of `batch` dn_cg_state records, (batch, 64) uint8."""
    return torch.zeros((int(batch), C.sizeof(_lib.DnCgState)), dtype=torch.uint8, device=device)


def poisson_cg_args(phase, x, r, p, q, dinv, state, workspace, tol=0.0, atol=0.0):
    """The argument struct of one dn_poisson_cg phase on FIXED buffers: x, r, p, q (B,...) float32 of n = numel / B nodes per sample,
    dinv the same or (1,...).  Returns (args, keep); launch it with poisson_cg_launch."""
    B = p.shape[0]
    n = p.numel() // B
    a = DnPoissonCgArgs()
    a.phase = CG_PHASES[phase] if isinstance(phase, str) else int(phase)
    a.batch, a.n = B, n
    keep = []
    for name, t in (("x", x), ("r", r), ("p", p), ("q", q), ("dinv", dinv)):
        if t is None:
            continue
        t = _require(t, name, None, True)
        if t.numel() not in ((n, B * n) if name == "dinv" else (B * n,)) or t.device != p.device:
            raise ValueError(f"{name} has shape {tuple(t.shape)}: expected {B} samples of {n} nodes on p's device")
        setattr(a, name, t.data_ptr())
        keep.append(t)
    if dinv is not None:
        a.dinv_batched = int(dinv.numel() == B * n)
    a.tol, a.atol = float(tol), float(atol)
    if state.dtype != torch.uint8 or state.numel() != B * C.sizeof(_lib.DnCgState) or not state.is_contiguous() or state.device != p.device:
        raise ValueError("state must be the (B, 64) uint8 block of poisson_cg_state on p's device")
    a.state = state.data_ptr()
    keep.append(state)
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
        keep.append(workspace)
    return a, keep


def poisson_cg_launch(args, device):
    """One dn_poisson_cg launch on the current stream of `device`."""
    rc = _lib.lib().dn_poisson_cg(C.byref(args), C.c_void_p(_raw_stream(device)))
    if rc:
        _lib.check(rc, "dn_poisson_cg")


def poisson_cg_phase(phase, x, r, p, q, dinv, state, workspace, tol=0.0, atol=0.0):
    """One phase of the PCG iteration (include/diffnet_hip.h: dn_poisson_cg) in place on x, r, p and the state block."""
    a, keep = poisson_cg_args(phase, x, r, p, q, dinv, state, workspace, tol, atol)
    poisson_cg_launch(a, p.device)


def poisson_cg_read_state(state):
    """The state block as a numpy record array (one synchronising copy)."""
    import numpy as np
    return state.cpu().numpy().view(np.dtype(CG_STATE_DTYPE)).reshape(-1)


# ---- PCG with a preconditioner that is a procedure (dn_poisson_pcg) and the multigrid transfers / smoother (dn_poisson_mg): raw wrappers
PCG_PHASES = {"resid0": _lib.PCG_RESID0, "update": _lib.PCG_UPDATE, "rz": _lib.PCG_RZ, "direction": _lib.PCG_DIRECTION}
MG_OPS = {"restrict": _lib.MG_RESTRICT, "prolong": _lib.MG_PROLONG, "smooth": _lib.MG_SMOOTH, "smooth0": _lib.MG_SMOOTH0}


def _flat_f32(t, name, numel, device):
    t = _require(t, name, None, True)
    if t.numel() not in (numel if isinstance(numel, tuple) else (numel,)) or t.device != device:
        raise ValueError(f"{name} has shape {tuple(t.shape)} on {t.device}: expected {numel} float32 values on {device}")
    return t


def poisson_pcg_args(phase, x, r, p, q, z, state, workspace, tol=0.0, atol=0.0):
    """The argument struct of one dn_poisson_pcg phase on FIXED buffers (include/diffnet_hip.h): the arrays the phase does not use may be
    None.  state: the (B, 64) block of poisson_cg_state, workspace: poisson_cg_workspace.  Returns (args, keep)."""
    B = int(state.shape[0])
    first = next(t for t in (r, p, x, q, z) if t is not None)
    n = first.numel() // B
    a = _lib.DnPoissonPcgArgs()
    a.phase = PCG_PHASES[phase] if isinstance(phase, str) else int(phase)
    a.batch, a.n = B, n
    keep = []
    for name, t in (("x", x), ("r", r), ("p", p), ("q", q), ("z", z)):
        if t is None:
            continue
        setattr(a, name, _flat_f32(t, name, B * n, first.device).data_ptr())
        keep.append(t)
    a.tol, a.atol = float(tol), float(atol)
    if state.dtype != torch.uint8 or state.numel() != B * C.sizeof(_lib.DnCgState) or not state.is_contiguous() or state.device != first.device:
        raise ValueError("state must be the (B, 64) uint8 block of poisson_cg_state on the arrays' device")
    a.state = state.data_ptr()
    keep.append(state)
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
        keep.append(workspace)
    return a, keep


def poisson_pcg_launch(args, device):
    rc = _lib.lib().dn_poisson_pcg(C.byref(args), C.c_void_p(_raw_stream(device)))
    if rc:
        _lib.check(rc, "dn_poisson_pcg")


def poisson_pcg_phase(phase, x, r, p, q, z, state, workspace, tol=0.0, atol=0.0):
    """One dn_poisson_pcg phase in place on x, r, p and the state block."""
    a, keep = poisson_pcg_args(phase, x, r, p, q, z, state, workspace, tol, atol)
    poisson_pcg_launch(a, state.device)


def poisson_mg_args(op, fine_shape, batch, x=None, b=None, q=None, dinv=None, c=None, mask=None, omega=1.0):
    """The argument struct of one dn_poisson_mg launch on FIXED buffers (include/diffnet_hip.h).  fine_shape: the node shape (memory
    order, z slowest) of the fine level -- of the only level for "smooth" / "smooth0".  x, b, q, dinv: (B,..) float32 of the fine level
    (dinv may be (1,..)); c: (B,..) of the coarse level; mask: uint8 image (B|1,..) of the coarse level for "restrict", of the fine
    level for "prolong".  Returns (args, keep)."""
    fine_shape = tuple(int(s) for s in fine_shape)
    nsd, B = len(fine_shape), int(batch)
    a = _lib.DnPoissonMgArgs()
    a.op = MG_OPS[op] if isinstance(op, str) else int(op)
    a.nsd, a.batch = nsd, B
    coarse_shape = tuple((s - 1) // 2 + 1 for s in fine_shape)
    for d, (sf, sc) in enumerate(zip(fine_shape[::-1], coarse_shape[::-1])):
        a.fine[d], a.coarse[d] = sf, sc
    for d in range(nsd, 3):
        a.fine[d] = a.coarse[d] = 1
    nf, nc = math.prod(fine_shape), math.prod(coarse_shape)
    first = next(t for t in (x, b, c) if t is not None)
    keep = []
    for name, t, numel in (("x", x, B * nf), ("b", b, B * nf), ("q", q, B * nf), ("dinv", dinv, (nf, B * nf)), ("c", c, B * nc)):
        if t is None:
            continue
        setattr(a, name, _flat_f32(t, name, numel, first.device).data_ptr())
        keep.append(t)
    if dinv is not None:
        a.dinv_batched = int(dinv.numel() == B * nf and B > 1)
    if mask is not None:
        nm = nc if a.op == _lib.MG_RESTRICT else nf
        if mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() not in (nm, B * nm) or mask.device != first.device:
            raise ValueError(f"mask must be a contiguous uint8 image of {nm} nodes, shared or per sample, on the arrays' device")
        a.mask, a.mask_batched = mask.data_ptr(), int(mask.numel() == B * nm and B > 1)
        keep.append(mask)
    a.omega = float(omega)
    return a, keep


def poisson_mg_launch(args, device):
    rc = _lib.lib().dn_poisson_mg(C.byref(args), C.c_void_p(_raw_stream(device)))
    if rc:
        _lib.check(rc, "dn_poisson_mg")


def poisson_mg(op, fine_shape, batch, **arrays):
    """One dn_poisson_mg launch (arguments as poisson_mg_args), in place on x (prolong, smooth, smooth0) or c (restrict)."""
    a, keep = poisson_mg_args(op, fine_shape, batch, **arrays)
    poisson_mg_launch(a, keep[0].device)


# ---- the transfers between meshes that need not be nested (dn_poisson_mg_transfer): the per-axis tables and the raw wrappers
def mg_general_coarse_shape(fine_shape):
    """The coarse node shape of dn_poisson_mg_transfer: an axis of e elements keeps ceil(e / 2)."""
    return tuple(int(s) // 2 + 1 for s in fine_shape)


def mg_axis_interpolation(n_src, n_dst):
    """Linear interpolation from a 1-D mesh of n_src nodes to one of n_dst nodes over the same length, from integers alone: node i of the
    target lies at the source coordinate i (n_src - 1) / (n_dst - 1) = j + rem / (n_dst - 1) and takes w0 = (n_dst - 1 - rem) / (n_dst - 1)
    of source node j and w1 = rem / (n_dst - 1) of node j + 1 (the last node: j = n_src - 2, w0 = 0, w1 = 1).  Returns (j int64 (n_dst,),
    w float32 (n_dst, 2)): each weight is a quotient of integers rounded to float32.  Pure: needs no GPU."""
    import numpy as np
    n_src, n_dst = int(n_src), int(n_dst)
    if n_src < 2 or n_dst < 2:
        raise ValueError("mg_axis_interpolation: both meshes need at least 2 nodes")
    num = np.arange(n_dst, dtype=np.int64) * (n_src - 1)
    j = num // (n_dst - 1)
    rem = num - j * (n_dst - 1)
    end = j > n_src - 2
    j, rem = np.where(end, n_src - 2, j), np.where(end, n_dst - 1, rem)
    w = np.stack([(n_dst - 1 - rem) / np.float64(n_dst - 1), rem / np.float64(n_dst - 1)], axis=1)
    return j, w.astype(np.float32)


MG_PARENT_DTYPE = [("j", "<i4"), ("w0", "<f4"), ("w1", "<f4"), ("pad", "<i4")]
MG_CHILDREN_DTYPE = [("first", "<i4"), ("count", "<i4"), ("pad", "<i4", (2,)), ("w", "<f4", (4,))]


def mg_axis_tables(nf, nc):
    """(parents, children) of one axis of dn_poisson_mg_transfer as numpy record arrays (include/diffnet_hip.h: dn_mg_parent,
    dn_mg_children): the rows and the columns of the same float32 1-D interpolation matrix.  Pure: needs no GPU."""
    import numpy as np
    nf, nc = int(nf), int(nc)
    if nf < 4 or nc != nf // 2 + 1:
        raise ValueError(f"mg_axis_tables: a fine axis of {nf} nodes (at least 4) has a coarse axis of {nf // 2 + 1} nodes, got {nc}")
    j, w = mg_axis_interpolation(nc, nf)
    parents = np.zeros(nf, MG_PARENT_DTYPE)
    parents["j"], parents["w0"], parents["w1"] = j, w[:, 0], w[:, 1]
    kids = [[] for _ in range(nc)]
    for i in range(nf):
        for t in (0, 1):
            if w[i, t] != 0:
                kids[j[i] + t].append((i, w[i, t]))
    children = np.zeros(nc, MG_CHILDREN_DTYPE)
    for jc, ks in enumerate(kids):
        # the children of coarse node jc lie strictly between its coarse neighbours: an open interval of 2 (nf - 1) / (nc - 1) <= 4 fine
        # spacings (nc - 1 = ceil((nf - 1) / 2)), which holds at most 4 integers -- and they are consecutive
        first = ks[0][0]
        assert 1 <= len(ks) <= 4 and [i for i, _ in ks] == list(range(first, first + len(ks))), (nf, nc, jc, ks)
        children["first"][jc], children["count"][jc] = first, len(ks)
        children["w"][jc, : len(ks)] = [wt for _, wt in ks]
    return parents, children


def mg_axis_matrix(parents, nc):
    """The float32 1-D interpolation matrix (nf, nc) that a parents table stands for (numpy)."""
    import numpy as np
    P = np.zeros((len(parents), nc), np.float32)
    rows = np.arange(len(parents))
    P[rows, parents["j"]] = parents["w0"]
    P[rows, parents["j"] + 1] += parents["w1"]
    return P


class MgTransferTables:
    """The per-axis device tables of dn_poisson_mg_transfer for one pair of levels.  fine_shape: node shape in memory order (z slowest);
    parents / children: lists of uint8 device tensors in the order x, y[, z]; matrices: the float32 1-D interpolation matrices
    (nf_d, nc_d) in MEMORY order of the axes, as device tensors (what the composed route multiplies by)."""

    def __init__(self, fine_shape, device):
        import numpy as np
        self.fine_shape = tuple(int(s) for s in fine_shape)
        self.coarse_shape = mg_general_coarse_shape(self.fine_shape)
        self.parents, self.children, mats = [], [], []
        for nf, nc in zip(self.fine_shape[::-1], self.coarse_shape[::-1]):
            p, c = mg_axis_tables(nf, nc)
            self.parents.append(torch.from_numpy(p.view(np.uint8).copy()).to(device))
            self.children.append(torch.from_numpy(c.view(np.uint8).copy()).to(device))
            mats.append(torch.from_numpy(mg_axis_matrix(p, nc)).to(device))
        self.matrices = mats[::-1]


def poisson_mg_transfer_args(op, fine_shape, batch, tables, x=None, b=None, q=None, c=None, mask=None):
    """The argument struct of one dn_poisson_mg_transfer launch on FIXED buffers (include/diffnet_hip.h).  fine_shape: the node shape
    (memory order, z slowest) of the fine level; tables: the `MgTransferTables` of it; arrays and mask as poisson_mg_args.  Returns
    (args, keep)."""
    fine_shape = tuple(int(s) for s in fine_shape)
    if tables.fine_shape != fine_shape:
        raise ValueError(f"the tables are those of a fine mesh of {tables.fine_shape} nodes, not {fine_shape}")
    nsd, B = len(fine_shape), int(batch)
    coarse_shape = tables.coarse_shape
    a = _lib.DnPoissonMgTransferArgs()
    a.op = MG_OPS[op] if isinstance(op, str) else int(op)
    a.nsd, a.batch = nsd, B
    for d, (sf, sc) in enumerate(zip(fine_shape[::-1], coarse_shape[::-1])):
        a.fine[d], a.coarse[d] = sf, sc
        a.parents[d], a.children[d] = tables.parents[d].data_ptr(), tables.children[d].data_ptr()
    for d in range(nsd, 3):
        a.fine[d] = a.coarse[d] = 1
    nf, nc = math.prod(fine_shape), math.prod(coarse_shape)
    first = next(t for t in (x, b, c) if t is not None)
    if tables.parents[0].device != first.device:
        raise ValueError("the tables live on another device than the arrays")
    keep = []
    for name, t, numel in (("x", x, B * nf), ("b", b, B * nf), ("q", q, B * nf), ("c", c, B * nc)):
        if t is None:
            continue
        setattr(a, name, _flat_f32(t, name, numel, first.device).data_ptr())
        keep.append(t)
    if mask is not None:
        nm = nc if a.op == _lib.MG_RESTRICT else nf
        if mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() not in (nm, B * nm) or mask.device != first.device:
            raise ValueError(f"mask must be a contiguous uint8 image of {nm} nodes, shared or per sample, on the arrays' device")
        a.mask, a.mask_batched = mask.data_ptr(), int(mask.numel() == B * nm and B > 1)
        keep.append(mask)
    keep.append(tables)
    return a, keep


def poisson_mg_transfer_launch(args, device):
    rc = _lib.lib().dn_poisson_mg_transfer(C.byref(args), C.c_void_p(_raw_stream(device)))
    if rc:
        _lib.check(rc, "dn_poisson_mg_transfer")


def poisson_mg_transfer(op, fine_shape, batch, tables=None, **arrays):
    """One dn_poisson_mg_transfer launch ("restrict" into c, "prolong" onto x); the tables are built when none are given."""
    first = next(t for t in (arrays.get(k) for k in ("x", "b", "c")) if t is not None)
    tables = MgTransferTables(fine_shape, first.device) if tables is None else tables
    a, keep = poisson_mg_transfer_args(op, fine_shape, batch, tables, **arrays)
    poisson_mg_transfer_launch(a, first.device)


class _CoefFn(torch.autograd.Function):
    """(g_nu, g_f) of one dn_poisson_coef_grad launch, differentiable wrt u and v -- the composed route it replaces can be differentiated
    twice, so this one can.  For cotangents (mu, mu_f):  <mu, g_nu> = a_nu <v, K_mu u~>  and  <mu_f, g_f> = a_f <v, M mu_f>  (K_mu the
    stiffness operator with coefficient mu, M the load operator), so the pullbacks are launches of the fused Poisson operator itself
    (`_fused`: they nest like _PoissonFn): to v, Z (a_nu K_mu u~ + a_f M mu_f); to u, a_nu Z K_mu v; with v absent the two collapse into
    the energy-gradient operator with (nu, f) := (a_nu mu, -a_f mu_f) and alpha = 2."""

    @staticmethod
    def forward(ctx, u, v, geom, dl, a_nu, a_f, wscale, want_nu, want_f):
        want = (("nu",) if want_nu else ()) + (("f",) if want_f else ())
        g_nu, g_f = poisson_coef_grad(geom, u, v, dl, a_nu, a_f, wscale, want)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(u, v)
        ctx.meta = (geom, dl, a_nu, a_f, wscale)
        return g_nu, g_f

    @staticmethod
    def backward(ctx, mu, mu_f):
        u, v = ctx.saved_tensors
        geom, dl, a_nu, a_f, wscale = ctx.meta
        gu = gv = None
        if mu is None and mu_f is None:
            return (None,) * 9
        mu = None if mu is None else mu.contiguous()
        mu_f = None if mu_f is None else mu_f.contiguous()
        if v is None:
            if ctx.needs_input_grad[0]:
                gu = _fused(geom, u, None if mu is None else a_nu * mu, None if mu_f is None else -a_f * mu_f, None, dl,
                            2.0 if mu is not None else 0.0, 1.0, 0.0, wscale, 1.0, 0.0)[0]
        else:
            if ctx.needs_input_grad[0] and mu is not None:
                hom = tuple(Dirichlet(d.mask, 0.0) for d in dl)
                gu = _fused(geom, v, mu, None, None, hom, a_nu, 0.0, 0.0, wscale, 1.0, 0.0)[0]
            if ctx.needs_input_grad[1]:
                gv = _fused(geom, u, mu, mu_f, None, dl, a_nu if mu is not None else 0.0, -a_f, 0.0, wscale, 1.0, 0.0)[0]
        return (gu, gv) + (None,) * 7


def _coef(geom, u, v, dl, a_nu, a_f, wscale, want_nu, want_f, in_scale=None):
    """poisson_coef_grad as a differentiable function of u, v and in_scale (autograd.Function where one of them requires a gradient -- a
    backward pass under create_graph --, the bare launch with the scale applied by the kernel otherwise)."""
    if _wants_grad(u, v, in_scale):
        g_nu, g_f = _CoefFn.apply(u, v, geom, tuple(dl), float(a_nu), float(a_f), float(wscale), bool(want_nu), bool(want_f))
        if in_scale is not None:
            g_nu = None if g_nu is None else g_nu * in_scale
            g_f = None if g_f is None else g_f * in_scale
        return g_nu, g_f
    want = (("nu",) if want_nu else ()) + (("f",) if want_f else ())
    return poisson_coef_grad(geom, u, v, dl, a_nu, a_f, wscale, want, in_scale)


def energy_loss_and_grads(geom, u, nu=None, f=None, dirichlet=(), c=1.0, jac=1.0, wrt=("u", "nu", "f")):
    """(loss, {"u": dloss/du, "nu": dloss/dnu, "f": dloss/df} restricted to `wrt`) of the energy loss from TWO launches, outside autograd:
    the fused operator (loss and u gradient) and dn_poisson_coef_grad (nu and f gradients) -- the optimiser-loop form, the sibling of
    energy_loss_and_grad.  A nu / f shared by the batch, shape (1,1,*N), receives the sum over the samples.  Q1 meshes."""
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    if any(w not in ("u", "nu", "f") for w in wrt):
        raise ValueError('wrt must name "u", "nu" and / or "f"')
    dl = tuple(_norm_dirichlet(dirichlet))
    B = u.shape[0]
    scale = 1.0 / (B * geom.nelem_total)
    ud = u.detach()
    nud = nu.detach() if isinstance(nu, torch.Tensor) else nu
    fd = f.detach() if isinstance(f, torch.Tensor) else f
    grad, _, loss = poisson_apply(geom, ud, nud, fd, None, dl, alpha=2.0 * c, beta=1.0, c=c, wscale=jac, out_scale=scale,
                                  want_out="u" in wrt, want_sums=True, loss_scale=scale)
    grads = {}
    if "u" in wrt:
        grads["u"] = grad
    want = tuple(w for w in ("nu", "f") if w in wrt)
    if want:
        g_nu, g_f = poisson_coef_grad(geom, ud, None, dl, scale * c, -scale, jac, want)
        for name, g, src in (("nu", g_nu, nud), ("f", g_f, fd)):
            if g is not None:
                if isinstance(src, torch.Tensor) and src.shape[0] != B:
                    g = g.sum(0, keepdim=True)
                grads[name] = g
    return loss, grads


class DeferredNorms:
    """Handle of a dn_fsdt_apply launch that left its partial sums of squares in the stream's FSDT reduction workspace (`defer_norms=True`): pass it
    as `norms_from` to the NEXT FSDT launch on that stream, which forms the norms itself.  Any other reducing FSDT launch in between overwrites the
    partials (the consumer's norms and outputs come out NaN); Poisson and Stokes launches use workspaces of their own and change nothing -- the
    pair is meant to be issued back to back (elasticity.fsdt_loss_and_grad, FsdtPlan)."""

    _next = [1]

    def __init__(self, ws, ticket=None):
        self.ws = ws
        if ticket is None:                     # a fresh ticket per deferring launch (1 .. 2^31 - 1)
            ticket = DeferredNorms._next[0]
            DeferredNorms._next[0] = ticket % 0x7FFFFFFE + 1
        self.ticket = ticket


def fsdt_apply(geom, w, phi_x, phi_y, bc=None, bc_values=(0.0, 0.0, 0.0), D11=1.0, D12=0.0, D22=1.0, D66=1.0, A44=1.0, A55=1.0,
               q=0.0, wscale=1.0, want_out=True, want_sums=True, in_scale=None, want_norms=False, in_num=None, in_den=None,
               defer_norms=False, norms_from=None):
    """One launch of dn_fsdt_apply (include/diffnet_hip.h): the three assembled FSDT plate residuals of the fields
    (B,1,ny,nx) and / or the float64 device tensor of their three sums of squares.  `bc`: Dirichlet node mask (fp32,
    `>= 0.5`, or bool/uint8), per sample or shared; `bc_values[k]`: float or tensor the k-th field / residual takes there;
    `in_scale`: optional float32 device tensor of 3 factors applied to the fields as they are loaded; `in_num` / `in_den`: the same
    with the factors in_num[k] / in_den[k] (0 where in_den[k] <= 0) formed by the kernel; `want_norms`: a third result, the float32
    tensor of the three Frobenius norms written by the same launch.  Returns (outs | None, sums | None[, norms]).
    `defer_norms` (round 4; instead of want_sums / want_norms): the launch leaves per-workgroup partials only -- no arrival protocol, no final
    reduction at its end (4.5-6.6 us of a 1025^2 launch) -- and the third result is a DeferredNorms handle; `norms_from=handle` (with in_num, without
    in_den) makes THIS launch form the norms from those partials, use them as in_den, and, with want_norms, return them as its third result.
    Calls on the same buffers reuse their prepared argument structs (small LRU, fresh outputs per call: see poisson_apply)."""
    if geom.nsd != 2:
        raise DiffNetHipError("fsdt_apply: 2-D meshes only")
    if defer_norms and (want_sums or want_norms or norms_from is not None):
        raise ValueError("fsdt_apply: defer_norms replaces want_sums / want_norms and does not combine with norms_from")
    if norms_from is not None and (in_num is None or in_den is not None or want_sums):
        raise ValueError("fsdt_apply: norms_from goes with in_num, without in_den and without want_sums")
    consts = tuple(float(x) for x in (D11, D12, D22, D66, A44, A55, q, wscale))
    # the key of the three-field flow operators, with one mask, no forcing and in_scale as the operator's own optional tensor
    key = _flow2d_key(geom, (w, phi_x, phi_y), (bc,), bc_values, (), consts, in_num, in_den,
                      (want_out, want_sums, want_norms, bool(defer_norms), None if norms_from is None else norms_from.ws.data_ptr()), (in_scale,))
    ent = _op_entry(_FSDT, key, _prepare_fsdt, (geom, w, phi_x, phi_y, bc, bc_values, consts, in_scale, in_num, in_den,
                                                (want_sums or want_norms or defer_norms) and norms_from is None, defer_norms, norms_from))
    dev = w.device
    outs = sums = norms = p0 = pair = None
    if want_out:
        o3 = torch.empty((3, *ent[4]), dtype=torch.float32, device=dev)      # one allocation, three views
        outs = list(o3.unbind(0))
        p0 = o3.data_ptr()
    if want_sums:
        sums = torch.empty(3, dtype=torch.float64, device=dev)
    if want_norms:
        norms = torch.empty(3, dtype=torch.float32, device=dev)
    if defer_norms:                  # the workspace the prepared call holds: _fsdt_patch puts the launch's handle in its place
        pair = [next(t for t in ent[5] if t.data_ptr() == ent[1].workspace)]
    _op_launch(_FSDT, ent, w, _fsdt_patch, ((p0, 4 * outs[0].numel() if want_out else 0, sums.data_ptr() if want_sums else None,
                                             norms.data_ptr() if want_norms else None), pair, norms_from))
    if defer_norms:
        return outs, None, pair[0]
    return (outs, sums, norms) if want_norms else (outs, sums)


def _fsdt_patch(args, ptrs):
    """_flow2d_patch and, per call, the ticket of a deferring launch (drawn here, under the operator's lock) and of the one it consumes."""
    out4, pair, norms_from = ptrs
    _flow2d_patch(args, out4)
    if pair is not None:
        pair[0] = DeferredNorms(pair[0])
        args.defer_sums = pair[0].ticket
    if norms_from is not None:
        args.den_ticket = norms_from.ticket


def _prepare_fsdt(geom, w, phi_x, phi_y, bc, bc_values, consts, in_scale, in_num, in_den, want_red, defer=False, norms_from=None):
    """Validation + argument struct of a dn_fsdt_apply call, outputs left unset: (mesh, args, tensors to keep alive, field shape)."""
    flds = [_require(t, n, 4) for t, n in ((w, "w"), (phi_x, "phi_x"), (phi_y, "phi_y"))]
    B = flds[0].shape[0]
    shape = (B, 1, *geom.node_shape)
    for t in flds:
        if tuple(t.shape) != shape:
            raise ValueError(f"fsdt_apply: field shape {tuple(t.shape)} != {shape}")
    keep = list(flds)
    args = DnFsdtArgs()
    args.w, args.phi_x, args.phi_y = (t.data_ptr() for t in flds)

    if bc is not None:
        if isinstance(bc, torch.Tensor) and not bc.is_cuda:
            raise DiffNetHipError("fsdt_apply: bc mask must be on the GPU")
        m, byte = _bc_mask(_FSDT, bc, 0)
        args.mask_is_u8 = 1 if byte else 0
        args.mask_batched = _nodal_batched(_FSDT, geom, B, m, "bc")
        args.bc_mask = m.data_ptr()
        keep.append(m)
        for k, v in enumerate(bc_values):
            if isinstance(v, torch.Tensor) and v.numel() > 1:
                v = _require(v, f"bc_values[{k}]")
                args.bc_field_batched[k] = _nodal_batched(_FSDT, geom, B, v, f"bc_values[{k}]")
                args.bc_field[k] = v.data_ptr()
                keep.append(v)
            else:
                args.bc_value[k] = float(v)
    args.D11, args.D12, args.D22, args.D66, args.A44, args.A55, args.q, args.wscale = consts
    mesh = geom.mesh_struct(B)
    for name, t in (("in_scale", in_scale), ("in_num", in_num), ("in_den", in_den)):
        if t is not None:
            t = _require(t, name, 1)
            if t.numel() != 3:
                raise ValueError(f"{name} must hold 3 floats")
            setattr(args, name, t.data_ptr())
            keep.append(t)
    if (in_num is None) != (in_den is None and norms_from is None) or (in_num is not None and in_scale is not None):
        raise ValueError("fsdt_apply: in_num and in_den (or norms_from) go together, and not with in_scale")
    if norms_from is not None:
        args.den_workspace = norms_from.ws.data_ptr()
        args.den_ticket = norms_from.ticket
        keep.append(norms_from.ws)
    args.defer_sums = 1 if defer else 0          # (the caller patches the pair's ticket in: fsdt_apply per call, FsdtPlan once)
    if want_red:
        ws = _op_workspace(_FSDT, mesh, B, flds[0].device)
        keep.append(ws)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    return mesh, args, keep, shape


class FsdtPlan:
    """The FSDT plate loss prepared once for FIXED buffers (the FSDT counterpart of PoissonPlan): `launch()` is two ctypes calls --
    dn_fsdt_apply on the fields (the three assembled residuals and, in the same launch, their Frobenius norms) and dn_fsdt_apply on the
    residuals as the VJP of sum_k weights[k] * ||R_k|| (the kernel forms weights[k] / ||R_k|| itself, 0 where a norm is 0) -- and returns
    (norms (3,) float32, [dL/dw, dL/dphi_x, dL/dphi_y]).  No autograd graph, no torch op, ~6 us of host time; outputs are overwritten by
    every launch.  `want_grad=False` prepares the first launch only.  Reference: e1_plate_bending_fsdt.py:128-232 (residuals, loss) and the
    backward pass autograd builds for it."""

    def __init__(self, geom, w, phi_x, phi_y, bc=None, bc_values=(0.0, 0.0, 0.0), weights=(1.0, 1.0, 1.0), want_grad=True,
                 D11=1.0, D12=0.0, D22=1.0, D66=1.0, A44=1.0, A55=1.0, q=0.0, wscale=1.0):
        if geom.nsd != 2:
            raise DiffNetHipError("FsdtPlan: 2-D meshes only")
        for t, n in ((w, "w"), (phi_x, "phi_x"), (phi_y, "phi_y")):
            _require(t, n, 4, True)          # strict: the plan keeps reading THESE buffers
        dev = w.device
        consts = tuple(float(x) for x in (D11, D12, D22, D66, A44, A55, q, wscale))
        self.mesh, self.args, self.keep, shape = _prepare_fsdt(geom, w, phi_x, phi_y, bc, bc_values, consts, None, None, None, True)
        self.residuals = torch.empty((3, *shape), dtype=torch.float32, device=dev)
        self.norms = torch.empty(3, dtype=torch.float32, device=dev)
        step = 4 * self.residuals[0].numel()
        for k in range(3):
            self.args.out[k] = self.residuals.data_ptr() + k * step
        self.args.norms = self.norms.data_ptr()
        self.grads = None
        self._refs = [(C.byref(self.mesh), C.byref(self.args))]
        if want_grad:
            self.weights = torch.tensor([float(x) for x in weights], dtype=torch.float32, device=dev)
            vconsts = consts[:6] + (0.0, consts[7])          # J = M K M, K symmetric: the VJP is the operator itself on the masked cotangents, q = 0
            R = list(self.residuals.unbind(0))
            # the first launch defers its sums: the second forms the norms from its partials (dn_fsdt_args.defer_sums / den_workspace) and writes them
            pair = DeferredNorms(next(t for t in self.keep if t.data_ptr() == self.args.workspace))
            self.vmesh, self.vargs, vkeep, _ = _prepare_fsdt(geom, R[0], R[1], R[2], bc, (0.0, 0.0, 0.0), vconsts, None, self.weights, None, False,
                                                             False, pair)
            self.vargs.norms = self.norms.data_ptr()
            self.args.norms = None
            self.args.defer_sums = pair.ticket
            self.keep += vkeep
            self.grads = torch.empty((3, *shape), dtype=torch.float32, device=dev)
            for k in range(3):
                self.vargs.out[k] = self.grads.data_ptr() + k * step
            self._refs.append((C.byref(self.vmesh), C.byref(self.vargs)))
        self.device = dev
        self.stream = _raw_stream(dev)           # the reduction workspace belongs to this stream
        self._fn = _lib.lib().dn_fsdt_apply
        self.result = (self.norms, None if self.grads is None else list(self.grads.unbind(0)))

    def launch(self):
        cur = _raw_stream(self.device)
        if cur != self.stream:
            raise DiffNetHipError("FsdtPlan.launch: prepared on another stream (its reduction workspace is per stream); prepare one plan per stream")
        s = C.c_void_p(cur)
        for mref, aref in self._refs:
            rc = self._fn(mref, aref, s)
            if rc:
                _lib.check(rc, "dn_fsdt_apply")
        return self.result



# ---- the host call path of the fused operators (poisson_apply, fsdt_apply, stokes_apply ... fdm_poisson_apply) --------------------
# Each operator has a reduction workspace of its OWN per (device, stream), never another operator's: an FSDT launch with defer_norms
# leaves its partials in its workspace for a later `norms_from` consumer, and a reducing launch of another operator issued in between must
# not overwrite them while the pair's ticket still matches (only FSDT's own reductions clear the ticket; another reducing FSDT launch in
# between clears it: NaN, never stale).  Launches on one stream are ordered, so they share the operator's workspace of that stream; a
# launch on another stream gets its own, and a prepared launch (PoissonPlan, FsdtPlan) keeps the one of the stream it was prepared on.
# _FusedOp holds an operator's workspaces, their sizes, its prepared-call cache and its launch lock; every one is listed in _FUSED_OPS
# (call_cache_clear).  What the calls share is written once, for any dimension: the workspace (_op_workspace), the look-up / prepare /
# cache step (_op_entry), the patch-under-lock / launch step (_op_launch), the check of a nodal field against the mesh
# (_nodal_batched), the form of a Dirichlet mask (_bc_mask) and a Gauss-point forcing tensor (_gp_forcing).
_FUSED_OPS = []


class _FusedOp:
    def __init__(self, name, args_type, meshless=False):
        self.name, self.args_type = name, args_type          # name: "stokes_apply", "ns_apply", ...: the prefix of its messages
        self.meshless = meshless           # the C entry points take no dn_mesh (a finite-difference grid: B, ny, nx in the arguments)
        self.fn, self.ws_fn = "dn_" + name, "dn_" + name.replace("_apply", "_workspace_bytes")      # the C entry points
        self.ws = {}
        self.ws_bytes = {}
        self.cache = __import__("collections").OrderedDict()
        self.launch_lock = _threading.Lock()
        self.entry = None                  # the bound C entry point (_op_launch)
        _FUSED_OPS.append(self)


_POISSON = _FusedOp("poisson_apply", DnPoissonArgs)      # its cache holds PoissonPlan objects, each with a lock of its own (poisson_apply)
_FSDT = _FusedOp("fsdt_apply", DnFsdtArgs)


def _op_workspace(op, mesh, B, dev):
    """The operator's reduction workspace on the current stream of `dev`, large enough for `mesh` under the launch plan in force."""
    key = (mesh.nx, mesh.ny, mesh.nz, mesh.degree, mesh.ngp, B)          # (nz is 1 on 2-D meshes and on no 3-D one)
    nbytes = op.ws_bytes.get(key)
    if nbytes is None:
        ws_fn = getattr(_lib.lib(), op.ws_fn)
        nbytes = ws_fn(B, mesh.ny, mesh.nx) if op.meshless else ws_fn(C.byref(mesh))
        if nbytes < 0:
            _lib.check(int(nbytes), op.ws_fn)
        op.ws_bytes[key] = nbytes
    key = (dev.index, _raw_stream(dev))
    with _WS_LOCK:
        ws = op.ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.zeros(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)   # ABI: zero-filled once
            op.ws[key] = ws
    return ws


def _op_entry(op, key, prepare, pargs):
    """The prepared call `key` (None: not cacheable) from the operator's cache, or prepare(*pargs) -- (mesh, args, tensors to keep alive,
    the field shape or the batch size) -- inserted into it: (mesh, args, their two references, shape | B, tensors kept alive)."""
    ent = None
    if key is not None:
        with _WS_LOCK:
            ent = op.cache.get(key)
            if ent is not None:
                op.cache.move_to_end(key)
    if ent is not None:
        _CALL_STATS["hit"] += 1
        return ent
    _CALL_STATS["miss" if key is not None else "uncached"] += 1
    mesh, args, keep, shape = prepare(*pargs)
    with _WS_LOCK:
        live_ws = list(op.ws.values())
    # an uncached call keeps its (possibly converted) tensors alive until it has been issued; a cached one only the workspace
    ent = (mesh, args, C.byref(mesh), C.byref(args), shape, keep if key is None else [t for t in keep if any(t is x for x in live_ws)])
    if key is not None:
        with _WS_LOCK:
            op.cache[key] = ent
            while len(op.cache) > _CALL_CACHE_MAX:
                op.cache.popitem(last=False)
    return ent


def _op_launch(op, ent, u, patch, ptrs):
    """patch(args, ptrs) sets the pointers of the call's fresh outputs in the (possibly shared, cached) argument struct; that and the
    launch are one step under the operator's lock.  The hit path of a call is host time: no closure, the entry point bound once."""
    fn = op.entry
    if fn is None:
        fn = op.entry = getattr(_lib.lib(), op.fn)
    with op.launch_lock:
        patch(ent[1], ptrs)
        rc = fn(ent[3], _stream(u)) if op.meshless else fn(ent[2], ent[3], _stream(u))
    if rc:
        _lib.check(rc, op.fn)


def _patch_out_sumsq_norm(args, ptrs):
    args.out, args.sumsq, args.norm = ptrs


def _nodal_batched(op, geom, B, t, what):
    """Checks the nodal field `t` (B | 1, ., *node_shape) against the mesh; 1 when it is per sample, 0 when shared."""
    nn = geom.nnode_total
    if tuple(t.shape[-geom.nsd:]) != tuple(geom.node_shape) or t.numel() not in (B * nn, nn):
        raise ValueError(f"{op.name}: {what} shape {tuple(t.shape)} does not match the mesh {(B, 1, *geom.node_shape)}")
    return 1 if (t.numel() == B * nn and B > 1) else 0


def _bc_mask(op, m, k):
    """The Dirichlet mask of condition k as the kernels read it: (a contiguous uint8 or fp32 tensor, whether it is the uint8 one)."""
    if not isinstance(m, torch.Tensor):
        raise TypeError(f"{op.name}: bc[{k}] must be a tensor or None (expand a PackedMask / BoxFaces to its image)")
    if not m.is_cuda:
        raise DiffNetHipError(f"{op.name}: bc[{k}] is on {m.device}: the FEM ops run on the GPU only (no CPU fallback)")
    if m.dtype in (torch.bool, torch.uint8):
        m = m.contiguous()
        return (m.view(torch.uint8) if m.dtype == torch.bool else m), True
    return _require(m, f"bc[{k}]"), False


def _gp_forcing(op, geom, keep, B, f, what):
    """A Gauss-point forcing tensor (B | 1, G, *elem_shape): (its pointer, 1 when it is per sample)."""
    f = _require(f, what)
    G, nel = geom.ngp_total, geom.nelem_total
    if tuple(f.shape[-1 - geom.nsd:]) != (G, *geom.elem_shape) or f.numel() not in (G * nel, B * G * nel):
        raise ValueError(f"{op.name}: {what} shape {tuple(f.shape)} is not (B | 1, {G}, {', '.join(str(n) for n in geom.elem_shape)})")
    keep.append(f)
    return f.data_ptr(), 1 if (f.numel() == B * G * nel and B > 1) else 0


# ---- the two three-field 2-D flow operators: dn_stokes_apply (PSPG) and dn_ns_apply (VMS residuals and their VJP) ------------------
_STOKES = _FusedOp("stokes_apply", DnStokesArgs)
_NS = _FusedOp("ns_apply", DnNsArgs)


def stokes_bc3(bc):
    """The three Dirichlet masks of a Stokes call: `bc` is one mask shared by u, v and p, or a sequence of three (None: no condition)."""
    if bc is None or isinstance(bc, torch.Tensor):
        return (bc, bc, bc)
    bc = tuple(bc)
    if len(bc) != 3:
        raise ValueError(f"stokes: bc must be one mask or three (got {len(bc)})")
    return bc


def stokes_f2(f_gp):
    """The two forcing terms of a Stokes call: None (no forcing), or a pair of None / float / Gauss-point tensor (Bf, G, nely, nelx)."""
    if f_gp is None:
        return (0.0, 0.0)
    f_gp = tuple(f_gp)
    if len(f_gp) != 2:
        raise ValueError(f"stokes: f_gp must be a pair (f1, f2) (got {len(f_gp)})")
    return tuple(0.0 if f is None else f for f in f_gp)


def _flow2d_check_mesh(op, geom):
    if geom.nsd != 2 or geom.deg != 1 or not 2 <= geom.ngp_1d <= 4:
        raise DiffNetHipError(f"{op.name}: 2-D Q1 meshes with 2..4 Gauss points per axis only (nsd {geom.nsd}, degree {geom.deg}, ngp {geom.ngp_1d})")


def _flow2d_key(geom, flds, bc3, vals, f2, consts, in_num, in_den, flags, cot=()):
    """Key of a cached prepared call (see _call_key) from the arguments the two operators share and the operator's own fields `cot`
    (each a tensor or None); None when an argument needs a conversion copy."""
    u, v, p = flds
    if not (all(isinstance(t, torch.Tensor) and t.is_cuda for t in flds) and tuple(u.shape[1:]) == (1, *geom.node_shape) and u.shape == v.shape == p.shape):
        return None
    parts = [geom.key, flds[0].device.index, _raw_stream(flds[0].device), consts, flags]
    for t in flds:
        k = _tkey(t)
        if k is None or k == 0 or k[1] != torch.float32:
            return None
        parts.append(k)
    for m in bc3:
        k = _tkey(m)
        if k is None or (k != 0 and k[1] not in (torch.float32, torch.uint8, torch.bool)):
            return None
        parts.append(k)
    for v in tuple(vals) + tuple(f2):
        if isinstance(v, torch.Tensor) and v.numel() > 1:
            k = _tkey(v)
            if k is None or k[1] != torch.float32:
                return None
            parts.append(k)
        else:
            parts.append(float(v))
    for t in (in_num, in_den):
        k = _tkey(t)
        if k is None or (k != 0 and (k[1] != torch.float32 or k[2] != (3,))):
            return None
        parts.append(k)
    for t in cot:
        k = _tkey(t)
        if k is None or (k != 0 and k[1] != torch.float32):
            return None
        parts.append(k)
    return tuple(parts)


def _flow2d_conditions(op, geom, args, keep, B, masks, vals, forcing):
    """The indexed members dn_stokes_args, dn_ns_args and dn_transport_args have in common: the masks into bc_mask[k] / mask_is_u8[k] /
    mask_batched[k], their values into bc_field[k] / bc_field_batched[k] or bc_value[k].  `forcing`: (name, float or Gauss-point tensor)
    pairs; returns (pointer | None, 1 when per sample, value) of each, for the caller's own members."""
    for k, m in enumerate(masks):
        if m is None:
            continue
        m, byte = _bc_mask(op, m, k)
        args.mask_is_u8[k] = 1 if byte else 0
        args.mask_batched[k] = _nodal_batched(op, geom, B, m, f"bc[{k}]")
        args.bc_mask[k] = m.data_ptr()
        keep.append(m)
    for k, val in enumerate(vals):
        if isinstance(val, torch.Tensor) and val.numel() > 1:
            if masks[k] is None:
                raise ValueError(f"{op.name}: bc_values[{k}] is a field but condition {k} has no mask")
            val = _require(val, f"bc_values[{k}]")
            args.bc_field_batched[k] = _nodal_batched(op, geom, B, val, f"bc_values[{k}]")
            args.bc_field[k] = val.data_ptr()
            keep.append(val)
        else:
            args.bc_value[k] = float(val)
    return [(*_gp_forcing(op, geom, keep, B, f, what), 0.0) if isinstance(f, torch.Tensor) and f.numel() > 1 else (None, 0, float(f))
            for what, f in forcing]


def _prepare_flow2d(op, geom, flds, bc3, vals, f2, in_num, in_den, want_red):
    """Validation + the members dn_stokes_args and dn_ns_args have in common (fields, masks, values, forcing, in_num / in_den, workspace),
    outputs left unset: (mesh, args, tensors to keep alive, field shape).  `flds`: (name, tensor) pairs, u, v, p first; any further ones
    are checked like them and head the keep list in the same order, for the caller to place."""
    name = op.name
    _flow2d_check_mesh(op, geom)
    flds = [_require(t, n, 4) for n, t in flds]
    B = flds[0].shape[0]
    shape = (B, 1, *geom.node_shape)
    for t in flds:
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: field shape {tuple(t.shape)} != {shape}")
    keep = list(flds)
    args = op.args_type()
    args.u, args.v, args.p = (t.data_ptr() for t in flds[:3])
    forcing = _flow2d_conditions(op, geom, args, keep, B, bc3, vals, [(f"f_gp[{k}]", f) for k, f in enumerate(f2)])
    for k, (ptr, per_sample, value) in enumerate(forcing):
        args.f_gp[k], args.f_batched[k], args.f_value[k] = ptr, per_sample, value
    if (in_num is None) != (in_den is None):
        raise ValueError(f"{name}: in_num and in_den go together")
    for what, t in (("in_num", in_num), ("in_den", in_den)):
        if t is not None:
            t = _require(t, what, 1)
            if t.numel() != 3:
                raise ValueError(f"{what} must hold 3 floats")
            setattr(args, what, t.data_ptr())
            keep.append(t)
    mesh = geom.mesh_struct(B)
    if want_red:
        ws = _op_workspace(op, mesh, B, flds[0].device)
        keep.append(ws)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    return mesh, args, keep, shape


def _flow2d_patch(args, ptrs):
    p0, step, args.sumsq, args.norms = ptrs
    if p0 is None:
        args.out[0] = args.out[1] = args.out[2] = None
    else:
        args.out[0], args.out[1], args.out[2] = p0, p0 + step, p0 + 2 * step


def _flow2d_call(op, key, prepare, pargs, u, want_out, want_sums, want_norms):
    """Look up the prepared call `key` (None: not cacheable) or prepare(*pargs) it, allocate fresh outputs, patch their three pointers
    into the (possibly shared, cached) argument struct and launch.  Returns (outs | None, sums | None[, norms])."""
    ent = _op_entry(op, key, prepare, pargs)
    dev = u.device
    outs = sums = norms = p0 = None
    if want_out:
        o3 = torch.empty((3, *ent[4]), dtype=torch.float32, device=dev)      # one allocation, three views
        outs = list(o3.unbind(0))
        p0 = o3.data_ptr()
    if want_sums:
        sums = torch.empty(3, dtype=torch.float64, device=dev)
    if want_norms:
        norms = torch.empty(3, dtype=torch.float32, device=dev)
    _op_launch(op, ent, u, _flow2d_patch, (p0, 4 * outs[0].numel() if want_out else 0, sums.data_ptr() if want_sums else None,
                                          norms.data_ptr() if want_norms else None))
    return (outs, sums, norms) if want_norms else (outs, sums)


def _prepare_stokes(geom, u, v, p, bc3, vals, f2, consts, in_num, in_den, want_red):
    """Validation + argument struct of a dn_stokes_apply call, outputs left unset: (mesh, args, tensors to keep alive, field shape)."""
    ent = _prepare_flow2d(_STOKES, geom, (("u", u), ("v", v), ("p", p)), bc3, vals, f2, in_num, in_den, want_red)
    args = ent[1]
    args.visco, args.pspg, args.wscale, transpose = consts
    args.transpose = 1 if transpose else 0
    return ent


def stokes_apply(geom, u, v, p, bc=None, bc_values=(0.0, 0.0, 0.0), visco=1.0, pspg=0.0, f_gp=None, wscale=1.0, want_out=True,
                 want_sums=True, want_norms=False, in_num=None, in_den=None, transpose=False):
    """One launch of dn_stokes_apply (include/diffnet_hip.h): the three assembled Stokes (PSPG) residuals of the fields u, v, p
    (B,1,ny,nx) and / or the float64 device tensor of their three sums of squares.  `bc`: one Dirichlet mask shared by the three fields or
    three (None: no condition), fp32 (`>= 0.5`) or bool / uint8, per sample or shared; `bc_values[k]`: float or tensor field k and
    residual k take there; `f_gp`: None or (f1, f2), each None, a float or a Gauss-point tensor (B | 1, G, nely, nelx); `in_num` / `in_den`:
    float32 device tensors of 3, field k is scaled by in_num[k] / in_den[k] (0 where in_den[k] <= 0) as it is loaded; `want_norms`: a third
    result, the float32 tensor of the three Frobenius norms written by the same launch; `transpose`: the adjoint J_R^T = S J_R S (forcing and
    Dirichlet values ignored).  Returns (outs | None, sums | None[, norms]).  Calls on the same buffers reuse their prepared argument structs
    (small LRU, fresh outputs per call: see poisson_apply)."""
    _flow2d_check_mesh(_STOKES, geom)
    bc3, f2, vals = stokes_bc3(bc), stokes_f2(f_gp), tuple(bc_values)
    if len(vals) != 3:
        raise ValueError("stokes_apply: bc_values must hold three entries")
    consts = (float(visco), float(pspg), float(wscale), bool(transpose))
    want_red = want_sums or want_norms
    key = _flow2d_key(geom, (u, v, p), bc3, vals, f2, consts, in_num, in_den, (want_out, want_sums, want_norms))
    return _flow2d_call(_STOKES, key, _prepare_stokes, (geom, u, v, p, bc3, vals, f2, consts, in_num, in_den, want_red),
                        u, want_out, want_sums, want_norms)


def _prepare_ns(geom, u, v, p, cot, bc3, vals, f2, consts, in_num, in_den, want_red):
    """Validation + argument struct of a dn_ns_apply call, outputs left unset: (mesh, args, tensors to keep alive, field shape)."""
    flds = [("u", u), ("v", v), ("p", p)]
    if cot is not None:
        flds += [(f"cot[{k}]", t) for k, t in enumerate(cot)]
    ent = _prepare_flow2d(_NS, geom, flds, bc3, vals, f2, in_num, in_den, want_red)
    if in_num is not None and cot is None:
        raise ValueError("ns_apply: in_num / in_den scale the cotangents of a VJP (cot)")
    args, keep = ent[1], ent[2]
    if cot is not None:
        for k in range(3):
            args.cot[k] = keep[3 + k].data_ptr()
    args.visco, args.wscale, args.tau_h[0], args.tau_h[1], args.cinv = consts
    args.vjp = 1 if cot is not None else 0
    return ent


def ns_apply(geom, u, v, p, bc=None, bc_values=(0.0, 0.0, 0.0), visco=1.0, f_gp=None, wscale=1.0, tau_h=None, cinv=36.0, cot=None,
             want_out=True, want_sums=True, want_norms=False, in_num=None, in_den=None):
    """One launch of dn_ns_apply (include/diffnet_hip.h): the three assembled Navier-Stokes (VMS) residuals of the fields u, v, p
    (B,1,ny,nx) and / or the float64 device tensor of their three sums of squares.  `bc`, `bc_values`, `f_gp`, `in_num` / `in_den`,
    `want_norms` as in stokes_apply; `tau_h`: the (hx, hy) of the stabilisation parameters (default: the mesh spacing); `cinv`: their
    constant.  `cot` (three fields like u): the VJP launch instead -- the gradient of sum_k <cot_k, R_k> with respect to (u, v, p) at the
    point (u, v, p), tau held fixed, with cot_k scaled by in_num[k] / in_den[k] where those are given.  Returns (outs | None, sums | None[,
    norms]).  Calls on the same buffers reuse their prepared argument structs (small LRU, fresh outputs per call: see poisson_apply)."""
    _flow2d_check_mesh(_NS, geom)
    bc3, f2, vals = stokes_bc3(bc), stokes_f2(f_gp), tuple(bc_values)
    if len(vals) != 3:
        raise ValueError("ns_apply: bc_values must hold three entries")
    if cot is not None:
        cot = tuple(cot)
        if len(cot) != 3:
            raise ValueError("ns_apply: cot must hold three fields")
    th = geom.hs[:2] if tau_h is None else tuple(tau_h)
    consts = (float(visco), float(wscale), float(th[0]), float(th[1]), float(cinv))
    want_red = want_sums or want_norms
    key = _flow2d_key(geom, (u, v, p), bc3, vals, f2, consts, in_num, in_den, (want_out, want_sums, want_norms),
                      cot if cot is not None else (None, None, None))
    return _flow2d_call(_NS, key, _prepare_ns, (geom, u, v, p, cot, bc3, vals, f2, consts, in_num, in_den, want_red),
                        u, want_out, want_sums, want_norms)


# ---- the one-field 2-D transport operator: dn_transport_apply (SUPG residual and its VJP) ------------------------------------------
# Its argument struct has the indexed members of the flow operators', for two conditions and one forcing term (_flow2d_conditions).
_TRANSPORT = _FusedOp("transport_apply", DnTransportArgs)


def transport_bc2(bc):
    """The two Dirichlet masks of a transport call: None, one mask (condition 1) or a pair (either may be None)."""
    if bc is None or isinstance(bc, torch.Tensor):
        return (bc, None)
    bc = tuple(bc)
    if len(bc) != 2:
        raise ValueError(f"transport: bc must be one mask or a pair (got {len(bc)})")
    return bc


def _transport_key(geom, u, nu, bc2, vals, f, consts, in_num, in_den, flags, cot):
    """Key of a cached prepared call (see _call_key); None when an argument needs a conversion copy."""
    if not (isinstance(u, torch.Tensor) and u.is_cuda and tuple(u.shape[1:]) == (1, *geom.node_shape)):
        return None
    parts = [geom.key, u.device.index, _raw_stream(u.device), consts, flags]
    k = _tkey(u)
    if k is None or k == 0 or k[1] != torch.float32:
        return None
    parts.append(k)
    for m in bc2:
        k = _tkey(m)
        if k is None or (k != 0 and k[1] not in (torch.float32, torch.uint8, torch.bool)):
            return None
        parts.append(k)
    for v in tuple(vals) + (f,):
        if isinstance(v, torch.Tensor) and v.numel() > 1:
            k = _tkey(v)
            if k is None or k[1] != torch.float32:
                return None
            parts.append(k)
        else:
            parts.append(float(v))
    for t in (nu, cot, in_num, in_den):
        k = _tkey(t)
        if k is None or (k != 0 and k[1] != torch.float32):
            return None
        parts.append(k)
    return tuple(parts)


def _prepare_transport(geom, u, nu, cot, bc2, vals, f, consts, in_num, in_den, want_red):
    """Validation + argument struct of a dn_transport_apply call, outputs left unset: (mesh, args, tensors to keep alive, field shape)."""
    name = _TRANSPORT.name
    _flow2d_check_mesh(_TRANSPORT, geom)
    args, keep = DnTransportArgs(), []
    u, B, shape = _elem_u(_TRANSPORT, geom, u, args, keep)
    if nu is not None:
        nu = _require(nu, "nu")
        args.nu_batched = _nodal_batched(_TRANSPORT, geom, B, nu, "nu")
        args.nu = nu.data_ptr()
        keep.append(nu)
    if cot is not None:
        cot = _require(cot, "cot", 4)
        if tuple(cot.shape) != shape:
            raise ValueError(f"{name}: cot shape {tuple(cot.shape)} != {shape}")
        args.cot = cot.data_ptr()
        keep.append(cot)
    elif in_num is not None:
        raise ValueError(f"{name}: in_num / in_den scale the cotangent of a VJP (cot)")
    args.vjp = 1 if cot is not None else 0
    (args.f_gp, args.f_batched, args.f_value), = _flow2d_conditions(_TRANSPORT, geom, args, keep, B, bc2, vals, [("f_gp", f)])
    if in_den is not None and in_num is None:
        raise ValueError(f"{name}: in_den needs in_num")
    for what, t in (("in_num", in_num), ("in_den", in_den)):
        if t is not None:
            t = _require(t, what)
            if t.numel() != 1:
                raise ValueError(f"{what} must hold one float")
            setattr(args, what, t.data_ptr())
            keep.append(t)
    (args.adv[0], args.adv[1], args.kappa[0], args.kappa[1], args.tau, args.react[0], args.react[1], args.react[2], args.react[3],
     args.wscale, first) = consts
    args.r_first_wins = 1 if first else 0
    mesh = geom.mesh_struct(B)
    if want_red:
        ws = _op_workspace(_TRANSPORT, mesh, B, u.device)
        keep.append(ws)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    return mesh, args, keep, shape


def transport_apply(geom, u, nu=None, bc=None, bc_values=(0.0, 0.0), r_first_wins=False, f_gp=None, adv=(0.0, 0.0), kappa=(1.0, 1.0),
                    tau=0.0, react=(0.0, 0.0, 0.0, 0.0), wscale=1.0, cot=None, want_out=True, want_sums=True, want_norm=False, in_num=None,
                    in_den=None):
    """One launch of dn_transport_apply (include/diffnet_hip.h): the assembled scalar transport (SUPG) residual of the field u
    (B,1,ny,nx) and / or the float64 device tensor (1,) of its sum of squares.  `nu`: None or a nodal coefficient field (B | 1,1,ny,nx);
    `bc`: None, one mask or a pair (either None), fp32 (`>= 0.5`) or bool / uint8, per sample or shared; `bc_values[k]`: float or tensor u
    and the residual take under condition k (where both hold, condition 2 wins on u; on the residual condition 1 if `r_first_wins`);
    `f_gp`: None, a float or a Gauss-point tensor (B | 1, G, nely, nelx); `adv`, `kappa`, `tau`, `react`: the coefficients.  `cot` (a field
    like u): the VJP launch instead -- the gradient of <cot, R> with respect to u at the point u, with cot scaled by in_num[0] (/ in_den[0])
    where those (float32 device tensors of 1) are given.  `want_norm`: a third result, the float32 tensor (1,) of the Frobenius norm written
    by the same launch.  Returns (out | None, sums | None[, norm]).  Calls on the same buffers reuse their prepared argument structs (small
    LRU, fresh outputs per call: see poisson_apply)."""
    _flow2d_check_mesh(_TRANSPORT, geom)
    bc2, vals = transport_bc2(bc), tuple(bc_values)
    if len(vals) != 2:
        raise ValueError("transport_apply: bc_values must hold two entries")
    adv, kappa, react = tuple(adv), tuple(kappa), tuple(react)
    if len(adv) != 2 or len(kappa) != 2 or len(react) != 4:
        raise ValueError("transport_apply: adv and kappa hold two entries, react four")
    f = 0.0 if f_gp is None else f_gp
    consts = (*(float(x) for x in adv), *(float(x) for x in kappa), float(tau), *(float(x) for x in react), float(wscale), bool(r_first_wins))
    want_red = want_sums or want_norm
    key = _transport_key(geom, u, nu, bc2, vals, f, consts, in_num, in_den, (want_out, want_sums, want_norm), cot)
    ent = _op_entry(_TRANSPORT, key, _prepare_transport, (geom, u, nu, cot, bc2, vals, f, consts, in_num, in_den, want_red))
    dev = u.device
    out = torch.empty(ent[4], dtype=torch.float32, device=dev) if want_out else None
    sums = torch.empty(1, dtype=torch.float64, device=dev) if want_sums else None
    norm = torch.empty(1, dtype=torch.float32, device=dev) if want_norm else None
    _op_launch(_TRANSPORT, ent, u, _patch_out_sumsq_norm, (out.data_ptr() if want_out else None, sums.data_ptr() if want_sums else None,
                                                          norm.data_ptr() if want_norm else None))
    return (out, sums, norm) if want_norm else (out, sums)


# ---- the element operators: dn_strongform_apply, dn_fosls_apply, dn_helmholtz_apply, dn_eikonal_apply on 2-D Q_P meshes and
# dn_eikonal3d_apply on 3-D Q1 meshes ----
# What their calls share beyond the above -- the key of a prepared call, the field u, the two conditions (dn_dirichlet bc[2]), the
# forcing, in_scale and the workspace -- is written once (_elem_*), with the number of mesh axes from geom.nsd; an operator's own
# functions name its own arguments and allocate its outputs.
_STRONGFORM = _FusedOp("strongform_apply", DnStrongformArgs)
_FOSLS = _FusedOp("fosls_apply", DnFoslsArgs)
_HELMHOLTZ = _FusedOp("helmholtz_apply", DnHelmholtzArgs)


def _elem2d_check_mesh(op, geom):
    if geom.nsd != 2 or geom.deg not in (1, 2, 3) or not 2 <= geom.ngp_1d <= 4 or (geom.deg > 1 and geom.ngp_1d < 3):
        raise DiffNetHipError(f"{op.name}: 2-D meshes of degree 1..3 with 2..4 Gauss points per axis (3 or 4 above degree 1) only "
                              f"(nsd {geom.nsd}, degree {geom.deg}, ngp {geom.ngp_1d})")
    if any((n - 1) % geom.deg for n in geom.sizes):
        raise ValueError(f"{op.name}: a degree-{geom.deg} mesh needs (n - 1) % {geom.deg} == 0 nodes per axis, got {geom.sizes}")


def _elem_key(parts, masks, scalars, optional):
    """Completes the key of a cached prepared call (see _call_key) that starts with `parts`: the masks (fp32 / uint8 / bool or None),
    the float-or-fp32-tensor arguments `scalars` and the optional fp32 tensors; None when an argument needs a conversion copy."""
    for m in masks:
        k = _tkey(m)
        if k is None or (k != 0 and k[1] not in (torch.float32, torch.uint8, torch.bool)):
            return None
        parts.append(k)
    for v in scalars:
        if isinstance(v, torch.Tensor) and v.numel() > 1:
            k = _tkey(v)
            if k is None or k[1] != torch.float32:
                return None
            parts.append(k)
        else:
            parts.append(float(v))
    for t in optional:
        k = _tkey(t)
        if k is None or (k != 0 and k[1] != torch.float32):
            return None
        parts.append(k)
    return tuple(parts)


def _elem_u_key(geom, u, consts, flags):
    """The head of the key of a call on one field u (B,1,*node_shape), or None."""
    if not (isinstance(u, torch.Tensor) and u.is_cuda and tuple(u.shape[1:]) == (1, *geom.node_shape)):
        return None
    k = _tkey(u)
    if k is None or k == 0 or k[1] != torch.float32:
        return None
    return [geom.key, u.device.index, _raw_stream(u.device), consts, flags, k]


def _elem_field(op, geom, args, keep, B, t, what, member):
    """A nodal fp32 field (B | 1, ., *node_shape) into args.<member> and args.<member>_batched."""
    t = _require(t, what)
    setattr(args, member + "_batched", _nodal_batched(op, geom, B, t, what))
    setattr(args, member, t.data_ptr())
    keep.append(t)


def _prepare_elem(op, geom, args, keep, B, dev, bc2, vals, f, f_gp, want_sums, in_scale=None, in_scale_on=None):
    """The members the element operators' argument structs have in common, after the operator's own: the two conditions, the forcing,
    in_scale (where the struct has one) and the workspace of a reducing call.  Returns the mesh struct."""
    name = op.name
    for k, m in enumerate(bc2):
        if m is None:
            continue
        m, byte = _bc_mask(op, m, k)
        d = args.bc[k]
        d.mask_kind = _lib.MASK_U8 if byte else _lib.MASK_F32
        d.mask_batched, d.mask = _nodal_batched(op, geom, B, m, f"bc[{k}]"), m.data_ptr()
        keep.append(m)
    for k, val in enumerate(vals):
        if isinstance(val, torch.Tensor) and val.numel() > 1:
            if bc2[k] is None:
                raise ValueError(f"{name}: bc_values[{k}] is a field but condition {k} has no mask")
            _elem_field(op, geom, args.bc[k], keep, B, val, f"bc_values[{k}]", "field")
        else:
            args.bc[k].value = float(val)
    if f is not None:
        if isinstance(f_gp, torch.Tensor) and f_gp.numel() > 1:
            raise ValueError(f"{name}: nodal forcing f and Gauss-point forcing f_gp exclude each other")
        _elem_field(op, geom, args, keep, B, f, "f", "f")
    elif isinstance(f_gp, torch.Tensor) and f_gp.numel() > 1:
        args.f_gp, args.f_batched = _gp_forcing(op, geom, keep, B, f_gp, "f_gp")
    else:
        args.f_value = float(f_gp)
    if in_scale is not None:
        in_scale = _require(in_scale, "in_scale")
        if in_scale.numel() != 1 or in_scale.device != dev:
            raise ValueError(f"{name}: in_scale must hold one float on {in_scale_on} device")
        args.in_scale = in_scale.data_ptr()
        keep.append(in_scale)
    mesh = geom.mesh_struct(B)
    if want_sums:
        ws = _op_workspace(op, mesh, B, dev)
        keep.append(ws)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    return mesh


def _elem_u(op, geom, u, args, keep):
    """The field u (B,1,*node_shape) of a one-field operator into args.u; returns (u, B, its shape)."""
    u = _require(u, "u", 2 + geom.nsd)
    B = u.shape[0]
    shape = (B, 1, *geom.node_shape)
    if tuple(u.shape) != shape:
        raise ValueError(f"{op.name}: field shape {tuple(u.shape)} != {shape}")
    keep.append(u)
    args.u = u.data_ptr()
    return u, B, shape


# ---- the fused 2-D strong-form least-squares loss and its gradient: dn_strongform_apply ----------------------------------------
def _strongform_key(geom, u, bc2, vals, f, f_gp, consts, in_scale, flags):
    parts = _elem_u_key(geom, u, consts, flags)
    return parts and _elem_key(parts, bc2, (*vals, f_gp), (f, in_scale))


def _prepare_strongform(geom, u, bc2, vals, f, f_gp, consts, in_scale, want_sum):
    """Validation + argument struct of a dn_strongform_apply call, outputs left unset: (mesh, args, tensors to keep alive, field shape)."""
    op = _STRONGFORM
    _elem2d_check_mesh(op, geom)
    args, keep = DnStrongformArgs(), []
    u, B, shape = _elem_u(op, geom, u, args, keep)
    args.ax, args.ay, args.b, args.dxx, args.dyy, args.fs, args.wscale, args.out_scale = consts
    for i in range(geom.ngp_1d):             # phi''(xi_ig) from the rule's own (truncated) abscissae, as the reference's tables
        for j in range(geom.deg + 1):
            args.d2basis[i][j] = geom.d2basis[i, j]
    mesh = _prepare_elem(op, geom, args, keep, B, u.device, bc2, vals, f, f_gp, want_sum, in_scale, "u's")
    return mesh, args, keep, shape


def _strongform_patch(args, ptrs):
    args.grad, args.sum = ptrs


def strongform_apply(geom, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, coef=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), wscale=1.0,
                     out_scale=1.0, in_scale=None, want_grad=True, want_sum=True):
    """One launch of dn_strongform_apply (include/diffnet_hip.h): sum_{b,e,g} W_g r_g^2 of the strong-form residual
    r = ax u_x + ay u_y + b u u_x + dxx u_xx + dyy u_yy + fs f of the field u (B,1,ny,nx) as a float64 device tensor (1,) and / or
    its gradient with respect to u times `out_scale` (times in_scale[0], a float32 device tensor of 1, where given).  `coef`:
    (ax, ay, b, dxx, dyy, fs); `bc`: None, one mask or a pair (either None), fp32 (`> 0.5`) or bool / uint8, per sample or shared;
    `bc_values[k]`: float or tensor u takes under condition k (where both hold, condition 2's); the forcing: a nodal field `f`
    (B | 1,1,ny,nx), or `f_gp`, a float or a Gauss-point tensor (B | 1, G, nely, nelx).  Degree 1..3.  Returns (grad | None, sum | None).
    Calls on the same buffers reuse their prepared argument structs (small LRU, fresh outputs per call: see poisson_apply)."""
    _elem2d_check_mesh(_STRONGFORM, geom)
    bc2, vals, coef = transport_bc2(bc), tuple(bc_values), tuple(float(x) for x in coef)
    if len(vals) != 2:
        raise ValueError("strongform_apply: bc_values must hold two entries")
    if len(coef) != 6:
        raise ValueError("strongform_apply: coef holds (ax, ay, b, dxx, dyy, fs)")
    if not (want_grad or want_sum):
        raise ValueError("strongform_apply: nothing to compute (want_grad and want_sum are both off)")
    fg = 0.0 if f_gp is None else f_gp
    consts = (*coef, float(wscale), float(out_scale))
    key = _strongform_key(geom, u, bc2, vals, f, fg, consts, in_scale, (want_grad, want_sum))
    ent = _op_entry(_STRONGFORM, key, _prepare_strongform, (geom, u, bc2, vals, f, fg, consts, in_scale, want_sum))
    grad = torch.empty(ent[4], dtype=torch.float32, device=u.device) if want_grad else None
    sums = torch.empty(1, dtype=torch.float64, device=u.device) if want_sum else None
    _op_launch(_STRONGFORM, ent, u, _strongform_patch, (grad.data_ptr() if want_grad else None, sums.data_ptr() if want_sum else None))
    return grad, sums


# ---- the fused 2-D first-order-system least-squares loss (u, mx, my) and its gradients: dn_fosls_apply --------------------------
def _fosls_key(geom, flds, packed, nu, bc2, vals, f, f_gp, consts, in_scale, flags):
    first = flds[0]
    if not (isinstance(first, torch.Tensor) and first.is_cuda):
        return None
    parts = [geom.key, first.device.index, _raw_stream(first.device), consts, flags, packed]
    for t in flds:
        k = _tkey(t)
        if k is None or k == 0 or k[1] != torch.float32 or tuple(k[2][1:]) != ((3 if packed else 1), *geom.node_shape):
            return None
        parts.append(k)
    return _elem_key(parts, bc2, (*vals, f_gp, nu), (f, in_scale))


def _prepare_fosls(geom, flds, packed, nu, bc2, vals, f, f_gp, consts, in_scale, want_sum):
    """Validation + argument struct of a dn_fosls_apply call, outputs left unset: (mesh, args, tensors to keep alive, batch size)."""
    op = _FOSLS
    name = op.name
    _elem2d_check_mesh(op, geom)
    nn = geom.nnode_total
    args = DnFoslsArgs()
    if packed:
        t = _require(flds[0], "fields", 4)
        B = t.shape[0]
        if tuple(t.shape) != (B, 3, *geom.node_shape):
            raise ValueError(f"{name}: fields shape {tuple(t.shape)} != {(B, 3, *geom.node_shape)} (channels u, mx, my)")
        keep = [t]
        args.u, args.mx, args.my = t.data_ptr(), t.data_ptr() + 4 * nn, t.data_ptr() + 8 * nn
        args.field_stride = 3 * nn
    else:
        keep = []
        B = flds[0].shape[0] if isinstance(flds[0], torch.Tensor) and flds[0].dim() == 4 else 0
        shape = (B, 1, *geom.node_shape)
        for what, t in zip(("u", "mx", "my"), flds):
            t = _require(t, what, 4)
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: field {what} shape {tuple(t.shape)} != {shape}")
            if t.device != flds[0].device:
                raise ValueError(f"{name}: the three fields must be on one device")
            setattr(args, what, t.data_ptr())
            keep.append(t)
        args.field_stride = nn
    dev = keep[0].device
    if isinstance(nu, torch.Tensor) and nu.numel() > 1:
        _elem_field(op, geom, args, keep, B, nu, "nu", "nu")
    else:
        args.nu_value = float(nu)
    args.wq, args.wd, args.fs, args.wscale, args.out_scale = consts
    mesh = _prepare_elem(op, geom, args, keep, B, dev, bc2, vals, f, f_gp, want_sum, in_scale, "the fields'")
    return mesh, args, keep, B


def _fosls_patch(args, ptrs):
    (args.grad_u, args.grad_mx, args.grad_my), args.grad_stride, args.sum = ptrs


def fosls_apply(geom, u=None, mx=None, my=None, nu=None, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, weights=(1.0, 1.0), fs=1.0,
                wscale=1.0, out_scale=1.0, in_scale=None, want_grad=True, want_sum=True, fields=None):
    """One launch of dn_fosls_apply (include/diffnet_hip.h): sum_{b,e,g} W_g (wq (qx^2 + qy^2) + wd d^2) of the first-order system
    qx = mx - nu u_x, qy = my - nu u_y, d = mx_x + my_y + fs f of the fields u, mx, my (B,1,ny,nx each) as a float64 device tensor (1,)
    and / or its gradients with respect to u, mx and my times `out_scale` (times in_scale[0], a float32 device tensor of 1, where
    given).  `fields`: instead of u, mx, my, one packed (B,3,ny,nx) tensor (channels u, mx, my), read in place; the gradient then is one
    packed (B,3,ny,nx) tensor.  `weights`: (wq, wd); `nu`: None (1), a float or a nodal field (B | 1,1,ny,nx); `bc`: None, one mask or a
    pair (either None) for u, fp32 (`> 0.5`) or bool / uint8, per sample or shared; `bc_values[k]`: float or tensor u takes under
    condition k (where both hold, condition 2's); the forcing: a nodal field `f` (B | 1,1,ny,nx), or `f_gp`, a float or a Gauss-point
    tensor (B | 1, G, nely, nelx).  `want_grad`: a bool, or with separate fields three bools (u, mx, my).  Degree 1..3.
    Returns ((gu, gmx, gmy) | packed gradient | None, sum | None); a gradient that was not asked for is None.
    Calls on the same buffers reuse their prepared argument structs (small LRU, fresh outputs per call: see poisson_apply)."""
    _elem2d_check_mesh(_FOSLS, geom)
    packed = fields is not None
    if packed and not (u is None and mx is None and my is None):
        raise ValueError("fosls_apply: pass either the packed `fields` or u, mx, my")
    if not packed and (u is None or mx is None or my is None):
        raise ValueError("fosls_apply: u, mx and my (or the packed `fields`) are required")
    bc2, vals, weights = transport_bc2(bc), tuple(bc_values), tuple(float(x) for x in weights)
    if len(vals) != 2:
        raise ValueError("fosls_apply: bc_values must hold two entries")
    if len(weights) != 2:
        raise ValueError("fosls_apply: weights holds (wq, wd)")
    want3 = (bool(want_grad),) * 3 if isinstance(want_grad, (bool, int)) else tuple(bool(x) for x in want_grad)
    if len(want3) != 3:
        raise ValueError("fosls_apply: want_grad is a bool or three of them (u, mx, my)")
    if packed and any(want3) != all(want3):
        raise ValueError("fosls_apply: a packed gradient holds all three channels; pass u, mx, my separately for a subset")
    if not (any(want3) or want_sum):
        raise ValueError("fosls_apply: nothing to compute (want_grad and want_sum are both off)")
    fg = 0.0 if f_gp is None else f_gp
    nuv = 1.0 if nu is None else nu
    consts = (*weights, float(fs), float(wscale), float(out_scale))
    flds = (fields,) if packed else (u, mx, my)
    key = _fosls_key(geom, flds, packed, nuv, bc2, vals, f, fg, consts, in_scale, (want3, want_sum))
    ent = _op_entry(_FOSLS, key, _prepare_fosls, (geom, flds, packed, nuv, bc2, vals, f, fg, consts, in_scale, want_sum))
    B = ent[4]
    dev = flds[0].device
    nn = geom.nnode_total
    if packed:
        grads = torch.empty((B, 3, *geom.node_shape), dtype=torch.float32, device=dev) if want3[0] else None
        ptrs = [grads.data_ptr() + 4 * nn * k if grads is not None else None for k in range(3)]
        gstride = 3 * nn
    else:
        grads = tuple(torch.empty((B, 1, *geom.node_shape), dtype=torch.float32, device=dev) if w else None for w in want3)
        ptrs = [g.data_ptr() if g is not None else None for g in grads]
        gstride = nn
        if not any(want3):
            grads = None
    sums = torch.empty(1, dtype=torch.float64, device=dev) if want_sum else None
    _op_launch(_FOSLS, ent, flds[0], _fosls_patch, (ptrs, gstride, sums.data_ptr() if want_sum else None))
    return grads, sums


# ---- the fused 2-D Helmholtz energy and weak-form residual: dn_helmholtz_apply ---------------------------------------------------
def _helmholtz_key(geom, u, nu, sigma, bc2, vals, f, f_gp, consts, flags):
    parts = _elem_u_key(geom, u, consts, flags)
    return parts and _elem_key(parts, bc2, (*vals, f_gp, sigma), (nu, f))


def _prepare_helmholtz(geom, u, nu, sigma, bc2, vals, f, f_gp, consts, want_sums):
    """Validation + argument struct of a dn_helmholtz_apply call, outputs left unset: (mesh, args, tensors to keep alive, field shape)."""
    op = _HELMHOLTZ
    _elem2d_check_mesh(op, geom)
    args, keep = DnHelmholtzArgs(), []
    u, B, shape = _elem_u(op, geom, u, args, keep)
    if nu is not None:
        _elem_field(op, geom, args, keep, B, nu, "nu", "nu")
    if isinstance(sigma, torch.Tensor) and sigma.numel() > 1:
        _elem_field(op, geom, args, keep, B, sigma, "sigma", "sigma")
    else:
        args.sigma_value = float(sigma)
    args.c, args.cr, args.fs, args.alpha, args.gamma, args.beta, args.wscale, args.out_scale = consts
    mesh = _prepare_elem(op, geom, args, keep, B, u.device, bc2, vals, f, f_gp, want_sums)
    return mesh, args, keep, shape


def _helmholtz_patch(args, ptrs):
    args.out, args.energy, args.sumsq = ptrs


def helmholtz_apply(geom, u, nu=None, sigma=0.0, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, energy_coef=(0.5, 0.5, 1.0),
                    out_coef=(1.0, 1.0, 1.0), wscale=1.0, out_scale=1.0, want_out=True, want_energy=True, want_sumsq=False):
    """One launch of dn_helmholtz_apply (include/diffnet_hip.h) on the field u (B,1,ny,nx):
    energy = sum W (c nu |grad u~|^2 - cr sg u~^2 - fs u~ f), `energy_coef` = (c, cr, fs);
    out = out_scale * zero_on_dirichlet(assembled W (alpha nu gradN . grad u~ - gamma sg N u~ - beta N f)), `out_coef` = (alpha, gamma,
    beta); sumsq = sum (out / out_scale)^2.  `nu`: None (1) or a nodal field (B | 1,1,ny,nx); `sigma`: a float or a nodal field likewise;
    `bc`: None, one mask or a pair (either None), fp32 (`> 0.5`) or bool / uint8, per sample or shared; `bc_values[k]`: float or tensor u
    takes under condition k (where both hold, condition 2's); the forcing: a nodal field `f` (B | 1,1,ny,nx), or `f_gp`, a float or a
    Gauss-point tensor (B | 1, G, nely, nelx).  Degree 1..3.  Returns (out | None, energy | None, sumsq | None), the two sums as float64
    device tensors (1,), unscaled.  Calls on the same buffers reuse their prepared argument structs (small LRU, fresh outputs per call:
    see poisson_apply)."""
    _elem2d_check_mesh(_HELMHOLTZ, geom)
    bc2, vals = transport_bc2(bc), tuple(bc_values)
    energy_coef, out_coef = tuple(float(x) for x in energy_coef), tuple(float(x) for x in out_coef)
    if len(vals) != 2:
        raise ValueError("helmholtz_apply: bc_values must hold two entries")
    if len(energy_coef) != 3 or len(out_coef) != 3:
        raise ValueError("helmholtz_apply: energy_coef holds (c, cr, fs), out_coef (alpha, gamma, beta)")
    if not (want_out or want_energy or want_sumsq):
        raise ValueError("helmholtz_apply: nothing to compute (want_out, want_energy and want_sumsq are all off)")
    fg = 0.0 if f_gp is None else f_gp
    sigma = 0.0 if sigma is None else sigma
    consts = (*energy_coef, *out_coef, float(wscale), float(out_scale))
    want_sums = want_energy or want_sumsq
    key = _helmholtz_key(geom, u, nu, sigma, bc2, vals, f, fg, consts, (want_out, want_sums))
    ent = _op_entry(_HELMHOLTZ, key, _prepare_helmholtz, (geom, u, nu, sigma, bc2, vals, f, fg, consts, want_sums))
    out = torch.empty(ent[4], dtype=torch.float32, device=u.device) if want_out else None
    sums = torch.empty(2, dtype=torch.float64, device=u.device) if want_sums else None
    _op_launch(_HELMHOLTZ, ent, u, _helmholtz_patch, (out.data_ptr() if want_out else None, sums.data_ptr() if want_energy else None,
                                                          sums.data_ptr() + 8 if want_sumsq else None))
    return out, (sums[0:1] if want_energy else None), (sums[1:2] if want_sumsq else None)


# ---- the fused eikonal weak-form residual and its VJP: dn_eikonal_apply (2-D Q_P meshes) and dn_eikonal3d_apply (3-D Q1 meshes) --------
# One argument struct (DnEikonalArgs) and one host path; what differs is the operator object and its mesh check.
_EIKONAL = _FusedOp("eikonal_apply", DnEikonalArgs)
_EIKONAL3D = _FusedOp("eikonal3d_apply", DnEikonalArgs)


def _eikonal3d_check_mesh(op, geom):
    if geom.nsd != 3:
        raise DiffNetHipError(f"{op.name}: 3-D meshes only (nsd {geom.nsd}); 2-D meshes: eikonal_apply")
    if geom.deg != 1 or not 2 <= geom.ngp_1d <= 4:
        raise DiffNetHipError(f"{op.name}: 3-D Q1 meshes with 2..4 Gauss points per axis only (degree {geom.deg}, ngp {geom.ngp_1d}); "
                              "any degree: eikonal.eikonal_residual_composed")


def _eikonal_key(geom, u, bc2, vals, f, f_gp, consts, cot, in_num, in_den, flags):
    parts = _elem_u_key(geom, u, consts, flags)
    if not parts:
        return None
    for t in (in_num, in_den):
        k = _tkey(t)
        if k is None or (k != 0 and k[2] != (1,)):
            return None
    return _elem_key(parts, bc2, (*vals, f_gp), (f, cot, in_num, in_den))


def _prepare_eikonal(op, check_mesh, geom, u, bc2, vals, f, f_gp, consts, cot, in_num, in_den, want_sums):
    """Validation + argument struct of a call of either eikonal operator, outputs left unset: (mesh, args, tensors to keep alive, field
    shape)."""
    check_mesh(op, geom)
    args, keep = DnEikonalArgs(), []
    u, B, shape = _elem_u(op, geom, u, args, keep)
    args.tau, args.sq, args.wscale = consts
    if cot is not None:
        cot = _require(cot, "cot", 2 + geom.nsd)
        if tuple(cot.shape) != shape or cot.device != u.device:
            raise ValueError(f"{op.name}: cotangent shape {tuple(cot.shape)} != {shape} (on u's device)")
        args.vjp, args.cot = 1, cot.data_ptr()
        keep.append(cot)
    for what, t in (("in_num", in_num), ("in_den", in_den)):
        if t is None:
            continue
        t = _require(t, what)
        if t.numel() != 1 or t.device != u.device:
            raise ValueError(f"{op.name}: {what} must hold one float on u's device")
        setattr(args, what, t.data_ptr())
        keep.append(t)
    mesh = _prepare_elem(op, geom, args, keep, B, u.device, bc2, vals, f, f_gp, want_sums)
    return mesh, args, keep, shape


def _eikonal_call(op, check_mesh, geom, u, bc, bc_values, f, f_gp, tau, sq, wscale, cot, in_num, in_den, want_out, want_sumsq, want_norm):
    """The body of eikonal_apply and eikonal3d_apply."""
    check_mesh(op, geom)
    bc2, vals = transport_bc2(bc), tuple(bc_values)
    if len(vals) != 2:
        raise ValueError(f"{op.name}: bc_values must hold two entries")
    if not (want_out or want_sumsq or want_norm):
        raise ValueError(f"{op.name}: nothing to compute (want_out, want_sumsq and want_norm are all off)")
    if cot is None and (in_num is not None or in_den is not None):
        raise ValueError(f"{op.name}: in_num / in_den scale the cotangent of a VJP launch (cot is None)")
    if in_den is not None and in_num is None:
        raise ValueError(f"{op.name}: in_den needs in_num")
    fg = 1.0 if f_gp is None else f_gp
    tau = float(tau)
    consts = (tau, 1.0 + tau if sq is None else float(sq), float(wscale))
    want_sums = want_sumsq or want_norm
    key = _eikonal_key(geom, u, bc2, vals, f, fg, consts, cot, in_num, in_den, (want_out, want_sums))
    ent = _op_entry(op, key, _prepare_eikonal, (op, check_mesh, geom, u, bc2, vals, f, fg, consts, cot, in_num, in_den, want_sums))
    out = torch.empty(ent[4], dtype=torch.float32, device=u.device) if want_out else None
    ss = torch.empty(1, dtype=torch.float64, device=u.device) if want_sumsq else None
    nrm = torch.empty(1, dtype=torch.float32, device=u.device) if want_norm else None
    _op_launch(op, ent, u, _patch_out_sumsq_norm, (out.data_ptr() if want_out else None, ss.data_ptr() if want_sumsq else None,
                                                  nrm.data_ptr() if want_norm else None))
    return out, ss, nrm


def eikonal_apply(geom, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=1.0, tau=0.0, sq=None, wscale=1.0, cot=None, in_num=None, in_den=None,
                  want_out=True, want_sumsq=False, want_norm=False):
    """One launch of dn_eikonal_apply (include/diffnet_hip.h) on the field u (B,1,ny,nx):
    R = zero_on_dirichlet(assembled W (tau u~ gradN . grad u~ + sq N |grad u~|^2 - N f)), `sq` None: 1 + tau; with `cot` (B,1,ny,nx) the
    launch is the VJP instead: the pullback of cot -- times in_num[0], divided by in_den[0] (float32 device tensors of 1) where given,
    zero on the Dirichlet nodes -- through R at u; it does not read the forcing.  `bc`: None, one mask or a pair (either None), fp32
    (`> 0.5`) or bool / uint8, per sample or shared; `bc_values[k]`: float or tensor u takes under condition k (where both hold,
    condition 2's); the forcing: a nodal field `f` (B | 1,1,ny,nx), or `f_gp`, a float (default 1) or a Gauss-point tensor
    (B | 1, G, nely, nelx).  Degree 1..3.  Returns (out | None, sumsq | None, norm | None): the sum of out^2 as a float64 device tensor
    (1,), its square root as a float32 one.  Calls on the same buffers reuse their prepared argument structs (small LRU, fresh outputs
    per call: see poisson_apply)."""
    return _eikonal_call(_EIKONAL, _elem2d_check_mesh, geom, u, bc, bc_values, f, f_gp, tau, sq, wscale, cot, in_num, in_den, want_out,
                         want_sumsq, want_norm)


def eikonal3d_apply(geom, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=1.0, tau=0.0, sq=None, wscale=1.0, cot=None, in_num=None, in_den=None,
                    want_out=True, want_sumsq=False, want_norm=False):
    """One launch of dn_eikonal3d_apply (include/diffnet_hip.h) on the field u (B,1,nz,ny,nx) of a 3-D Q1 mesh: the 3-D twin of
    `eikonal_apply`, with the same arguments and results.
    R = zero_on_dirichlet(assembled W (N (sq |grad u~|^2 - f) + tau u~ gradN . grad u~)), `sq` None: 1 + tau; with `cot` (B,1,nz,ny,nx)
    the launch is the VJP instead: the pullback of cot -- times in_num[0], divided by in_den[0] (float32 device tensors of 1) where
    given, zero on the Dirichlet nodes -- through R at u; it does not read the forcing.  `bc`: None, one mask or a pair (either None),
    fp32 (`> 0.5`) or bool / uint8, per sample or shared; `bc_values[k]`: float or tensor u takes under condition k (where both hold,
    condition 2's); the forcing: a nodal field `f` (B | 1,1,nz,ny,nx), or `f_gp`, a float (default 1) or a Gauss-point tensor
    (B | 1, G, nelz, nely, nelx) in the order of `gauss_pt_evaluation`.  Returns (out | None, sumsq | None, norm | None): the sum of
    out^2 as a float64 device tensor (1,), its square root as a float32 one.  Calls on the same buffers reuse their prepared argument
    structs; the reduction workspace is the operator's own, one per stream."""
    return _eikonal_call(_EIKONAL3D, _eikonal3d_check_mesh, geom, u, bc, bc_values, f, f_gp, tau, sq, wscale, cot, in_num, in_den, want_out,
                         want_sumsq, want_norm)


# ---- the fused 2-D finite-difference Poisson residual, its sums and its gradient: dn_fdm_poisson_apply --------------------------
_FDM_POISSON = _FusedOp("fdm_poisson_apply", DnFdmPoissonArgs, meshless=True)
_FDM_KERNELS = {}


class _FdmGrid:
    """What the shared argument checks ask of a geometry, for a finite-difference grid of ny x nx nodes (it has no element tables)."""
    nsd = 2

    def __init__(self, ny, nx):
        self.node_shape, self.nnode_total = (ny, nx), ny * nx


def fdm_default_kernels(nx):
    """(kx, ky, kxx, kyy), nine floats each, row-major: the 'fdm' kernels of get_deriv_kernels for a domain of `nx` nodes -- the values of
    DiffNetFDM's sobelx / sobely / sobelxx / sobelyy parameters."""
    ks = _FDM_KERNELS.get(nx)
    if ks is None:
        from .fdm import get_deriv_kernels
        _, kx, ky, _, _, kxx, kyy, _ = get_deriv_kernels(2, "fdm", 3, nx)
        ks = _FDM_KERNELS[nx] = tuple(tuple(float(v) for v in k.astype("float32").reshape(-1)) for k in (kx, ky, kxx, kyy))
    return ks


def _fdm_k9(k):
    if isinstance(k, tuple) and len(k) == 9 and all(type(v) is float for v in k):
        return k
    v = torch.as_tensor(k, dtype=torch.float32).reshape(-1).tolist()
    if len(v) != 9:
        raise ValueError(f"fdm_poisson_apply: a kernel holds 3 x 3 values, got {len(v)}")
    return tuple(v)


def _fdm_poisson_key(u, nu_t, f_t, bc2, vals, consts, in_scale, flags):
    if not (isinstance(u, torch.Tensor) and u.is_cuda):
        return None
    k = _tkey(u)
    if k is None or k == 0 or k[1] != torch.float32:
        return None
    return _elem_key(["fdm", u.device.index, _raw_stream(u.device), consts, flags, k], bc2, vals, (nu_t, f_t, in_scale))


def _prepare_fdm_poisson(u, nu_t, f_t, bc2, vals, consts, in_scale, want_sums):
    """Validation + argument struct of a dn_fdm_poisson_apply call, outputs left unset: (grid, args, tensors to keep alive, field shape)."""
    op = _FDM_POISSON
    args, keep = DnFdmPoissonArgs(), []
    u = _require(u, "u", 4)
    B, ch, ny, nx = u.shape
    if ch != 1 or ny < 3 or nx < 3:
        raise ValueError(f"{op.name}: u must be (B,1,ny,nx) with ny, nx >= 3, got {tuple(u.shape)}")
    grid = _FdmGrid(ny, nx)
    keep.append(u)
    args.u, args.B, args.ny, args.nx = u.data_ptr(), B, ny, nx
    ks, args.fs, args.out_scale, args.nbc_scale, args.nu_value, args.f_value = consts
    args.kx[:], args.ky[:], args.kxx[:], args.kyy[:] = ks
    if nu_t is not None:
        _elem_field(op, grid, args, keep, B, nu_t, "nu", "nu")
    if f_t is not None:
        _elem_field(op, grid, args, keep, B, f_t, "f", "f")
    for k, m in enumerate(bc2):
        if m is None:
            continue
        m, byte = _bc_mask(op, m, k)
        d = args.bc[k]
        d.mask_kind = _lib.MASK_U8 if byte else _lib.MASK_F32
        d.mask_batched, d.mask = _nodal_batched(op, grid, B, m, f"bc[{k}]"), m.data_ptr()
        keep.append(m)
    for k, val in enumerate(vals):
        if isinstance(val, torch.Tensor) and val.numel() > 1:
            if bc2[k] is None:
                raise ValueError(f"{op.name}: bc_values[{k}] is a field but condition {k} has no mask")
            _elem_field(op, grid, args.bc[k], keep, B, val, f"bc_values[{k}]", "field")
        else:
            args.bc[k].value = float(val)
    if in_scale is not None:
        in_scale = _require(in_scale, "in_scale")
        if in_scale.numel() != B or in_scale.device != u.device:
            raise ValueError(f"{op.name}: in_scale must hold one float per sample ({B}) on u's device")
        args.in_scale = in_scale.data_ptr()
        keep.append(in_scale)
    mesh = DnMesh()                          # no element tables: only what keys the workspace size
    mesh.nsd, mesh.batch, mesh.nx, mesh.ny, mesh.nz = 2, B, nx, ny, 1
    if want_sums:
        ws = _op_workspace(op, mesh, B, u.device)
        keep.append(ws)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    return mesh, args, keep, (B, 1, ny, nx)


def _fdm_poisson_patch(args, ptrs):
    args.grad, args.sums, args.res = ptrs


def fdm_poisson_apply(u, nu=None, f=None, bc=None, bc_values=(0.0, 0.0), kernels=None, fs=1.0, out_scale=1.0, nbc_scale=0.0, in_scale=None,
                      want_res=False, want_grad=True, want_sums=True):
    """One launch of dn_fdm_poisson_apply (include/diffnet_hip.h) on the field u (B,1,ny,nx) of a finite-difference grid: the residual
    r = fs f + (kx * u~)(kx * nu) + (ky * u~)(ky * nu) + nu (kxx * u~ + kyy * u~) on the interior, `*` the valid 3x3 correlation of
    nn.functional.conv2d and u~ the field after the two conditions.  Returns (grad | None, sums | None, res | None):
    res (B,1,ny-2,nx-2); sums (B,3) float64 per sample: sum r^2, sum_x (u~[0,x] - u~[1,x])^2, sum_x (u~[ny-1,x] - u~[ny-2,x])^2;
    grad (B,1,ny,nx) = out_scale (in_scale[b] d(sum r^2)/du + nbc_scale d(the two row sums)/du), zero on the Dirichlet nodes
    (`in_scale`: a float32 device tensor of B, or None for 1).  `nu`: a tensor (B | 1,1,ny,nx), a float, or None for 1; `f`: likewise,
    None for 0.  `bc`: None, one mask or a pair (either None), fp32 (`> 0.5`) or bool / uint8, per sample or shared; `bc_values[k]`:
    float or tensor u takes under condition k (where both hold, condition 2's).  `kernels`: (kx, ky, kxx, kyy), 3x3 each, any values;
    None: the 'fdm' kernels of get_deriv_kernels for nx.  Calls on the same buffers reuse their prepared argument structs (small LRU,
    fresh outputs per call: see poisson_apply); the reduction workspace is the operator's own, one per stream."""
    op = _FDM_POISSON
    bc2, vals = transport_bc2(bc), tuple(bc_values)
    if len(vals) != 2:
        raise ValueError("fdm_poisson_apply: bc_values must hold two entries")
    if not (want_res or want_grad or want_sums):
        raise ValueError("fdm_poisson_apply: nothing to compute (want_res, want_grad and want_sums are all off)")
    if not isinstance(u, torch.Tensor) or u.dim() != 4:
        raise ValueError("fdm_poisson_apply: u must be a tensor (B,1,ny,nx)")
    if kernels is None:
        ks = fdm_default_kernels(u.shape[3])
    else:
        ks = tuple(_fdm_k9(k) for k in kernels)
        if len(ks) != 4:
            raise ValueError("fdm_poisson_apply: kernels holds (kx, ky, kxx, kyy)")
    nu_t, nu_v = (nu, 0.0) if isinstance(nu, torch.Tensor) else (None, 1.0 if nu is None else float(nu))
    f_t, f_v = (f, 0.0) if isinstance(f, torch.Tensor) else (None, 0.0 if f is None else float(f))
    consts = (ks, float(fs), float(out_scale), float(nbc_scale), nu_v, f_v)
    key = _fdm_poisson_key(u, nu_t, f_t, bc2, vals, consts, in_scale, (want_res, want_grad, want_sums))
    ent = _op_entry(op, key, _prepare_fdm_poisson, (u, nu_t, f_t, bc2, vals, consts, in_scale, want_sums))
    B, _, ny, nx = ent[4]
    grad = torch.empty(ent[4], dtype=torch.float32, device=u.device) if want_grad else None
    sums = torch.empty((B, 3), dtype=torch.float64, device=u.device) if want_sums else None
    res = torch.empty((B, 1, ny - 2, nx - 2), dtype=torch.float32, device=u.device) if want_res else None
    _op_launch(op, ent, u, _fdm_poisson_patch, (grad.data_ptr() if want_grad else None, sums.data_ptr() if want_sums else None,
                                                res.data_ptr() if want_res else None))
    return grad, sums, res


def compute_winding_nodes(points, normals, area, q):
    """Drop-in for `compute_winding_nodes` of IBN/poisson-2d/parametric/IBN_2D.py:89-104 (same argument shapes:
    points / normals (B,1,Npts,2), area (B,1,Npts,1) -- unused by the reference too --, q = stack((xx, yy)) (2,Ny,Nx));
    returns (B,1,Nx,Ny).  One HIP launch instead of a Python loop over grid columns."""
    pts = _require(points.reshape(points.size(0), -1, 2), "points")
    nrm = _require(normals.reshape(normals.size(0), -1, 2), "normals")
    nodes = _require(q if q.is_cuda else q.to(pts.device), "nodes", 3)
    B, npts = pts.shape[0], pts.shape[1]
    ny, nx = nodes.shape[1], nodes.shape[2]
    out = torch.empty((B, 1, nx, ny), dtype=torch.float32, device=pts.device)
    rc = _lib.lib().dn_winding_nodes(_p(pts), _p(nrm), _p(nodes), _p(out), B, npts, ny, nx, _stream(pts))
    _lib.check(rc, "dn_winding_nodes")
    return out


WINDING_TILES = (1, 2, 4)        # queries per thread dn_winding_field can be told to use (0: picked from the problem size)
WINDING_CHUNK = 256              # points staged in LDS per pass
WINDING_THREADS = 256            # threads per workgroup: a workgroup owns WINDING_THREADS * tile queries
_WINDING_METRICS = {"l1": 0, "l2": 1, 0: 0, 1: 1}


def winding_field(points, normals, area, queries, metric="l1", power=3, scale=1.0, threshold=0.5, want_field=True, want_mask=False,
                  tile=0):
    """w[b, q] = scale * sum_p area[b, p] ((x_p - q) . n_p) / dist(x_p - q)^power on a flat list of queries (dn_winding_field): one launch.
    points, normals (B, Np, dim), dim 2 or 3; area (B, Np) / (B, Np, 1) or None (= 1); queries (dim, nq) or (dim, *grid), coordinate-major,
    shared by all samples, on the points' device or on the host; metric "l1" (the reference's quirk) or "l2"; power 2 or 3.
    Returns (field, mask): the float32 field (B, nq) if want_field, else None, and the uint8 mask (B, nq) = (w > threshold), compared
    in the kernel, if want_mask, else None.  Every tensor must be float32 and contiguous.  Not differentiable: nothing is recorded for
    autograd (the reference only thresholds the field); winding_field_vjp is its vector-Jacobian product, diffnet_amd.winding wires the two."""
    named = [("points", points), ("normals", normals), ("queries", queries)] + ([("area", area)] if area is not None else [])
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"winding_field: {name} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"winding_field: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"winding_field: {name} must be contiguous")
    if points.dim() != 3 or points.shape[2] not in (2, 3):
        raise ValueError(f"winding_field: points must be (B, Np, 2) or (B, Np, 3), got {tuple(points.shape)}")
    B, npts, dim = points.shape
    if normals.shape != points.shape:
        raise ValueError(f"winding_field: normals {tuple(normals.shape)} do not match points {tuple(points.shape)}")
    if area is not None and tuple(area.shape) not in ((B, npts), (B, npts, 1)):
        raise ValueError(f"winding_field: area must be (B, Np) or (B, Np, 1) = ({B}, {npts}[, 1]), got {tuple(area.shape)}")
    if queries.dim() < 2 or queries.shape[0] != dim:
        raise ValueError(f"winding_field: queries must be ({dim}, nq) or ({dim}, *grid), got {tuple(queries.shape)}")
    if metric not in _WINDING_METRICS:
        raise ValueError(f"winding_field: metric must be 'l1' or 'l2', got {metric!r}")
    if power not in (2, 3):
        raise ValueError(f"winding_field: power must be 2 or 3, got {power!r}")
    if tile not in (0,) + WINDING_TILES:
        raise ValueError(f"winding_field: tile must be 0 (automatic) or one of {WINDING_TILES}, got {tile!r}")
    if not (want_field or want_mask):
        raise ValueError("winding_field: nothing to compute (want_field and want_mask are both off)")
    for name, t in named:
        if t.device != points.device and not (name == "queries" and t.device.type == "cpu"):
            raise ValueError(f"winding_field: {name} is on {t.device}, points on {points.device}")
    if not points.is_cuda:
        raise DiffNetHipError(f"points are on {points.device}: winding_field runs on the GPU only (no CPU fallback); move them with .cuda()")
    nq = queries[0].numel()
    if B < 1 or npts < 1 or nq < 1:
        raise ValueError(f"winding_field: empty problem (B = {B}, Np = {npts}, nq = {nq})")
    qd = queries if queries.is_cuda else queries.to(points.device)
    field = torch.empty((B, nq), dtype=torch.float32, device=points.device) if want_field else None
    mask = torch.empty((B, nq), dtype=torch.uint8, device=points.device) if want_mask else None
    rc = _lib.lib().dn_winding_field(_p(points), _p(normals), _p(area), _p(qd), _p(field), _p(mask), B, npts, nq, dim, _WINDING_METRICS[metric],
                                     power, float(scale), float(threshold), tile, _stream(points))
    _lib.check(rc, "dn_winding_field")
    return field, mask


WINDING_VJP_MAX_SLICES = 1024    # most slices of the query range dn_winding_field_vjp takes (0: picked from the problem size)
_WINDING_VJP_WANT = ("points", "normals", "area")


def winding_field_vjp(points, normals, area, queries, grad_field, metric="l1", power=3, scale=1.0, want=_WINDING_VJP_WANT, slices=0):
    """The vector-Jacobian product of winding_field with respect to the cloud (dn_winding_field_vjp; queries are constants): with
    d = x_p - q, num = d . n_p and the cotangent g = grad_field (B, nq),
        grad_area = scale sum_q g num inv,   grad_normals_i = scale a_p sum_q g d_i inv,   grad_points_i = scale a_p sum_q g (n_i inv + num dinv_i).
    Arguments as winding_field: every tensor float32 and contiguous, on the GPU, queries (dim, nq) or (dim, *grid) possibly on the host.
    want: the subset of ("points", "normals", "area") to compute; "area" needs an area.  slices: 0 picks the split of the query range
    from the problem size, 1..1024 force it (the bits are repeatable for a given value and the same for every `want`).
    Returns (grad_points | None, grad_normals | None, grad_area | None); grad_area has the shape the area was given in."""
    named = [("points", points), ("normals", normals), ("queries", queries), ("grad_field", grad_field)] + ([("area", area)] if area is not None else [])
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"winding_field_vjp: {name} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"winding_field_vjp: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"winding_field_vjp: {name} must be contiguous")
    if points.dim() != 3 or points.shape[2] not in (2, 3):
        raise ValueError(f"winding_field_vjp: points must be (B, Np, 2) or (B, Np, 3), got {tuple(points.shape)}")
    B, npts, dim = points.shape
    if normals.shape != points.shape:
        raise ValueError(f"winding_field_vjp: normals {tuple(normals.shape)} do not match points {tuple(points.shape)}")
    if area is not None and tuple(area.shape) not in ((B, npts), (B, npts, 1)):
        raise ValueError(f"winding_field_vjp: area must be (B, Np) or (B, Np, 1) = ({B}, {npts}[, 1]), got {tuple(area.shape)}")
    if queries.dim() < 2 or queries.shape[0] != dim:
        raise ValueError(f"winding_field_vjp: queries must be ({dim}, nq) or ({dim}, *grid), got {tuple(queries.shape)}")
    nq = queries[0].numel()
    if grad_field.dim() != 2 or tuple(grad_field.shape) != (B, nq):
        raise ValueError(f"winding_field_vjp: grad_field must be (B, nq) = ({B}, {nq}), got {tuple(grad_field.shape)}")
    if metric not in _WINDING_METRICS:
        raise ValueError(f"winding_field_vjp: metric must be 'l1' or 'l2', got {metric!r}")
    if power not in (2, 3):
        raise ValueError(f"winding_field_vjp: power must be 2 or 3, got {power!r}")
    if not isinstance(slices, int) or not 0 <= slices <= WINDING_VJP_MAX_SLICES:
        raise ValueError(f"winding_field_vjp: slices must be 0 (automatic) or 1..{WINDING_VJP_MAX_SLICES}, got {slices!r}")
    want = tuple(want)
    if not want or any(w not in _WINDING_VJP_WANT for w in want):
        raise ValueError(f"winding_field_vjp: want must be a non-empty subset of {_WINDING_VJP_WANT}, got {want!r}")
    if "area" in want and area is None:
        raise ValueError("winding_field_vjp: the gradient with respect to the area was asked for, but no area was given")
    for name, t in named:
        if t.device != points.device and not (name == "queries" and t.device.type == "cpu"):
            raise ValueError(f"winding_field_vjp: {name} is on {t.device}, points on {points.device}")
    if not points.is_cuda:
        raise DiffNetHipError(f"points are on {points.device}: winding_field_vjp runs on the GPU only (no CPU fallback); the composed "
                              "route for CPU tensors is diffnet_amd.winding.winding_field_composed")
    if B < 1 or npts < 1 or nq < 1:
        raise ValueError(f"winding_field_vjp: empty problem (B = {B}, Np = {npts}, nq = {nq})")
    h = _lib.lib()
    qd = queries if queries.is_cuda else queries.to(points.device)
    s = min(slices or h.dn_winding_field_vjp_slices(B, npts, nq), (nq + WINDING_CHUNK - 1) // WINDING_CHUNK)
    ws, ws_bytes = None, 0
    if s > 1:
        ws_bytes = h.dn_winding_field_vjp_workspace_bytes(B, npts, dim, s)
        _lib.check(min(ws_bytes, 0), "dn_winding_field_vjp_workspace_bytes")
        ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=points.device)
    gp = torch.empty_like(points) if "points" in want else None
    gn = torch.empty_like(points) if "normals" in want else None
    ga = torch.empty_like(area) if "area" in want else None
    rc = h.dn_winding_field_vjp(_p(points), _p(normals), _p(area), _p(qd), _p(grad_field), _p(gp), _p(gn), _p(ga), _p(ws), ws_bytes, B, npts, nq,
                                dim, _WINDING_METRICS[metric], power, float(scale), s, _stream(points))
    _lib.check(rc, "dn_winding_field_vjp")
    return gp, gn, ga


# ---- the fused point-cloud terms: evaluation at points, penalty loss and gradient: dn_points_apply ----------------------------------
_POINTS = _FusedOp("points_apply", DnPointsArgs)
_POINTS_KINDS = {"none": _lib.POINTS_NONE, "dot": _lib.POINTS_DOT, "match": _lib.POINTS_MATCH}


def _points_check_mesh(op, geom):
    if geom.nsd not in (2, 3) or geom.deg != 1:
        raise DiffNetHipError(f"{op.name}: Q1 meshes only (nsd {geom.nsd}, degree {geom.deg}); any degree: points.point_terms_composed")


def _points_key(geom, B, npts, consts, flags, f32s, i32s):
    dev = next(t for t in f32s + i32s if t is not None).device
    parts = [geom.key, B, npts, dev.index, _raw_stream(dev), consts, flags]
    for ts, dt in ((f32s, torch.float32), (i32s, torch.int32)):
        for t in ts:
            k = _tkey(t)
            if k is None or (k != 0 and k[1] != dt):
                return None
            parts.append(k)
    return tuple(parts)


def _prepare_points(geom, B, npts, consts, flags, f32s, i32s):
    """Validation + argument struct of a dn_points_apply call, fresh outputs left unset: (mesh, args, tensors to keep alive, batch)."""
    op = _POINTS
    _points_check_mesh(op, geom)
    u, xi, target, normals, cot, gscale_dev, grad_out = f32s
    elem, offsets = i32s
    dscale, kind, target_value, w_val, w_nrm, gscale = consts
    penalty, want_sums, accumulate = flags
    args, keep = DnPointsArgs(), []
    T, nsd = B * npts, geom.nsd
    dev = xi.device
    node_shape = (B, 1, *geom.node_shape)

    def put(member, t, what, numel, dtype=torch.float32, shape=None):
        if t is None:
            return
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev:
            raise DiffNetHipError(f"{op.name}: {what} must be a tensor on {dev} (the fused point terms run on the GPU only)")
        if t.dtype != dtype or not t.is_contiguous():
            raise TypeError(f"{op.name}: {what} must be a contiguous {dtype} tensor, got {t.dtype}")
        if t.numel() != numel or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f"{op.name}: {what} holds {tuple(t.shape)}, expected {shape or numel} values")
        setattr(args, member, t.data_ptr())
        keep.append(t)

    put("u", u, "u", B * geom.nnode_total, shape=node_shape)
    put("xi", xi, "xi", nsd * T)
    put("elem", elem, "elem", T, torch.int32)
    put("offsets", offsets, "offsets", B * geom.nelem_total + 1, torch.int32)
    put("target", target, "target", T)
    put("normals", normals, "normals", nsd * T)
    put("cot", cot, "cot", (1 + nsd) * T)
    put("gscale_dev", gscale_dev, "gscale_dev", 1)
    put("grad", grad_out, "grad_out", B * geom.nnode_total, shape=node_shape)
    args.npts, args.kind, args.penalty, args.accumulate = npts, kind, int(penalty), int(accumulate)
    args.dscale[:] = dscale
    args.target_value, args.w_val, args.w_nrm, args.gscale = target_value, w_val, w_nrm, gscale
    mesh = geom.mesh_struct(B)
    if want_sums:
        ws = _op_workspace(op, mesh, B, dev)
        keep.append(ws)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    return mesh, args, keep, B


def _points_patch(args, ptrs):
    values, pgrads, sums, cot, grad = ptrs
    args.values, args.pgrads, args.sums = values, pgrads, sums
    if cot is not None:
        args.cot = cot
    if grad is not None:
        args.grad = grad


def points_apply(geom, batch, npts, xi, elem=None, offsets=None, u=None, dscale=(1.0, 1.0, 1.0), kind="none", penalty=False, target=None,
                 normals=None, w_val=1.0, w_nrm=1.0, want_values=False, want_pgrads=False, want_sums=False, want_cot=False, cot=None,
                 want_grad=False, grad_out=None, accumulate=False, gscale=1.0, gscale_dev=None):
    """One call of dn_points_apply (include/diffnet_hip.h) on the sorted point list of a `points.PointPlan` (B = batch samples of npts
    points; T = B npts): xi (nsd, T) float32, elem (T) int32, offsets (B nel + 1) int32, in the kernels' axis order (x, y[, z]).
    Forward launch (needs u (B,1,*node_shape) and elem) when values, pgrads or the penalty are asked for: values (T), pgrads (nsd, T);
    `penalty`: sums (3 float64: value term, normals term, total; `want_sums`) and the per-point cotangents cot (1 + nsd, T)
    (`want_cot`), from `target` (a float or a (T) tensor), `normals` (nsd, T), `kind` "none" | "dot" | "match", w_val, w_nrm.
    Adjoint launch (needs offsets) when `want_grad`: the pullback of `cot` -- the one just computed, or the tensor passed in -- times
    gscale (and gscale_dev[0], a float32 device tensor of 1), into a fresh tensor, into `grad_out`, or added to `grad_out` with
    `accumulate`.  Returns (values, pgrads, sums, cot, grad), None where not asked for.  Calls on the same buffers reuse their prepared
    argument structs (small LRU, fresh outputs per call: see poisson_apply)."""
    op = _POINTS
    _points_check_mesh(op, geom)
    if kind not in _POINTS_KINDS:
        raise ValueError(f"{op.name}: kind must be one of {sorted(_POINTS_KINDS)}, got {kind!r}")
    if not isinstance(xi, torch.Tensor) or not xi.is_cuda:
        raise DiffNetHipError(f"{op.name}: the fused point terms run on the GPU only (no CPU fallback): points.point_terms_composed is the torch route")
    if not (want_values or want_pgrads or penalty or want_grad):
        raise ValueError(f"{op.name}: nothing to compute")
    if penalty and not (want_sums or want_cot or want_grad):
        raise ValueError(f"{op.name}: a penalty needs want_sums, want_cot or want_grad")
    if (want_sums or want_cot) and not penalty:
        raise ValueError(f"{op.name}: sums and cot are results of the penalty")
    if want_grad and not penalty and cot is None:
        raise ValueError(f"{op.name}: the adjoint needs per-point cotangents (cot, or a penalty in the same call)")
    if accumulate and (grad_out is None or not want_grad):
        raise ValueError(f"{op.name}: accumulate adds to grad_out")
    if penalty and cot is not None:
        raise ValueError(f"{op.name}: cot is an input of an adjoint-only call")
    B, npts, dev = int(batch), int(npts), xi.device
    if B * npts == 0 and not (want_sums or want_grad):          # nothing per point and nothing else: no launch
        e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        return e(0) if want_values else None, e(geom.nsd, 0) if want_pgrads else None, None, e(1 + geom.nsd, 0) if want_cot else None, None
    tt, tv = (target, 0.0) if isinstance(target, torch.Tensor) else (None, 0.0 if target is None else float(target))
    ds = tuple(float(x) for x in dscale) + (1.0,) * (3 - len(dscale))
    consts = (ds, _POINTS_KINDS[kind], tv, float(w_val), float(w_nrm), float(gscale))
    flags = (bool(penalty), bool(want_sums), bool(accumulate), want_values, want_pgrads, want_cot, want_grad)
    f32s = (u, xi, tt, normals if penalty else None, cot, gscale_dev, grad_out if want_grad else None)
    i32s = (elem, offsets if want_grad else None)
    key = _points_key(geom, B, npts, consts, flags, f32s, i32s)
    ent = _op_entry(op, key, _prepare_points, (geom, B, npts, consts, flags[:3], f32s, i32s))
    T, nsd = B * npts, geom.nsd
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)      # noqa: E731
    values = new(T) if want_values else None
    pgrads = new(nsd, T) if want_pgrads else None
    sums = new(3, dtype=torch.float64) if want_sums else None
    cot_new = new(1 + nsd, T) if penalty and (want_cot or want_grad) else None
    grad = new(B, 1, *geom.node_shape) if want_grad and grad_out is None else None
    _op_launch(op, ent, xi, _points_patch, tuple(None if t is None else t.data_ptr() for t in (values, pgrads, sums, cot_new, grad)))
    return values, pgrads, sums, cot_new if want_cot else None, (grad_out if grad is None else grad) if want_grad else None
