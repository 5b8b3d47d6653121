"""ctypes binding of libdiffnet_hip.so (the C ABI declared in include/diffnet_hip.h).

The library is the product: there is no CPU fallback.  `lib()` raises if the shared object is
missing or does not export the full ABI.  Loading needs no GPU (symbols are checked on CPU boxes
too); compute entry points need device pointers.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DN_LIB_PATH") or os.path.join(HERE, "libdiffnet_hip.so")     # DN_LIB_PATH: another build of the library
ABI_VERSION = 10

DN_E = {-1: "DN_E_BADARG", -2: "DN_E_UNSUPPORTED", -3: "DN_E_WORKSPACE", -4: "DN_E_HANDOVER"}


class DnMesh(C.Structure):
    _fields_ = [("nsd", C.c_int32), ("degree", C.c_int32), ("ngp", C.c_int32), ("batch", C.c_int32),
                ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("scale", C.c_float * 3), ("gpw", C.c_float * 4),
                ("basis", (C.c_float * 4) * 4), ("dbasis", (C.c_float * 4) * 4)]


class DnDirichlet(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("field", C.c_void_p), ("value", C.c_float),
                ("mask_kind", C.c_int32), ("mask_batched", C.c_int32), ("field_batched", C.c_int32),
                ("box_faces", C.c_int32), ("row_words", C.c_int32)]


MASK_F32, MASK_U8, MASK_BITS, MASK_BOX = 0, 1, 2, 3
FACE_XLO, FACE_XHI, FACE_YLO, FACE_YHI, FACE_ZLO, FACE_ZHI = 1, 2, 4, 8, 16, 32


class DnPoissonArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("nu", C.c_void_p), ("f", C.c_void_p), ("f_gp", C.c_void_p),
                ("nu_batched", C.c_int32), ("f_batched", C.c_int32),
                ("bc", DnDirichlet * 2),
                ("alpha", C.c_float), ("beta", C.c_float), ("c", C.c_float), ("wscale", C.c_float),
                ("out_scale", C.c_float),
                ("out", C.c_void_p), ("energy", C.c_void_p), ("sumsq", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("energy_f32", C.c_void_p), ("energy_scale", C.c_double), ("strip_select", C.c_int32), ("accumulate_sums", C.c_int32), ("defer_sums", C.c_int32),
                ("fold_prev", C.c_void_p), ("f_is_load", C.c_int32)]


class DnFsdtArgs(C.Structure):
    _fields_ = [("w", C.c_void_p), ("phi_x", C.c_void_p), ("phi_y", C.c_void_p),
                ("bc_mask", C.c_void_p), ("mask_is_u8", C.c_int32), ("mask_batched", C.c_int32),
                ("bc_field", C.c_void_p * 3), ("bc_field_batched", C.c_int32 * 3), ("bc_value", C.c_float * 3),
                ("D11", C.c_float), ("D12", C.c_float), ("D22", C.c_float), ("D66", C.c_float), ("A44", C.c_float),
                ("A55", C.c_float), ("q", C.c_float), ("wscale", C.c_float),
                ("out", C.c_void_p * 3), ("sumsq", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("in_scale", C.c_void_p), ("norms", C.c_void_p), ("in_num", C.c_void_p), ("in_den", C.c_void_p),
                ("defer_sums", C.c_int32), ("den_ticket", C.c_int32), ("den_workspace", C.c_void_p)]


class DnStokesArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("v", C.c_void_p), ("p", C.c_void_p),
                ("bc_mask", C.c_void_p * 3), ("mask_is_u8", C.c_int32 * 3), ("mask_batched", C.c_int32 * 3),
                ("bc_field", C.c_void_p * 3), ("bc_field_batched", C.c_int32 * 3), ("bc_value", C.c_float * 3),
                ("f_gp", C.c_void_p * 2), ("f_batched", C.c_int32 * 2), ("f_value", C.c_float * 2),
                ("visco", C.c_float), ("pspg", C.c_float), ("wscale", C.c_float), ("transpose", C.c_int32),
                ("out", C.c_void_p * 3), ("sumsq", C.c_void_p), ("norms", C.c_void_p), ("in_num", C.c_void_p), ("in_den", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class DnNsArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("v", C.c_void_p), ("p", C.c_void_p),
                ("bc_mask", C.c_void_p * 3), ("mask_is_u8", C.c_int32 * 3), ("mask_batched", C.c_int32 * 3),
                ("bc_field", C.c_void_p * 3), ("bc_field_batched", C.c_int32 * 3), ("bc_value", C.c_float * 3),
                ("f_gp", C.c_void_p * 2), ("f_batched", C.c_int32 * 2), ("f_value", C.c_float * 2),
                ("visco", C.c_float), ("wscale", C.c_float), ("tau_h", C.c_float * 2), ("cinv", C.c_float), ("vjp", C.c_int32),
                ("cot", C.c_void_p * 3),
                ("out", C.c_void_p * 3), ("sumsq", C.c_void_p), ("norms", C.c_void_p), ("in_num", C.c_void_p), ("in_den", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class DnTransportArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("nu", C.c_void_p), ("nu_batched", C.c_int32), ("r_first_wins", C.c_int32),
                ("bc_mask", C.c_void_p * 2), ("mask_is_u8", C.c_int32 * 2), ("mask_batched", C.c_int32 * 2),
                ("bc_field", C.c_void_p * 2), ("bc_field_batched", C.c_int32 * 2), ("bc_value", C.c_float * 2),
                ("f_gp", C.c_void_p), ("f_batched", C.c_int32), ("f_value", C.c_float),
                ("adv", C.c_float * 2), ("kappa", C.c_float * 2), ("tau", C.c_float), ("react", C.c_float * 4), ("wscale", C.c_float),
                ("vjp", C.c_int32),
                ("cot", C.c_void_p), ("out", C.c_void_p), ("sumsq", C.c_void_p), ("norm", C.c_void_p),
                ("in_num", C.c_void_p), ("in_den", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class DnStrongformArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("f", C.c_void_p), ("f_gp", C.c_void_p), ("f_batched", C.c_int32), ("f_value", C.c_float),
                ("bc", DnDirichlet * 2),
                ("ax", C.c_float), ("ay", C.c_float), ("b", C.c_float), ("dxx", C.c_float), ("dyy", C.c_float), ("fs", C.c_float),
                ("wscale", C.c_float), ("out_scale", C.c_float), ("d2basis", (C.c_float * 4) * 4),
                ("in_scale", C.c_void_p), ("grad", C.c_void_p), ("sum", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class DnFoslsArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("mx", C.c_void_p), ("my", C.c_void_p), ("field_stride", C.c_int64),
                ("nu", C.c_void_p), ("nu_batched", C.c_int32), ("nu_value", C.c_float),
                ("f", C.c_void_p), ("f_gp", C.c_void_p), ("f_batched", C.c_int32), ("f_value", C.c_float),
                ("bc", DnDirichlet * 2),
                ("wq", C.c_float), ("wd", C.c_float), ("fs", C.c_float), ("wscale", C.c_float), ("out_scale", C.c_float),
                ("in_scale", C.c_void_p), ("grad_u", C.c_void_p), ("grad_mx", C.c_void_p), ("grad_my", C.c_void_p), ("grad_stride", C.c_int64),
                ("sum", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class DnHelmholtzArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("nu", C.c_void_p), ("sigma", C.c_void_p), ("f", C.c_void_p), ("f_gp", C.c_void_p),
                ("nu_batched", C.c_int32), ("sigma_batched", C.c_int32), ("f_batched", C.c_int32),
                ("sigma_value", C.c_float), ("f_value", C.c_float),
                ("bc", DnDirichlet * 2),
                ("c", C.c_float), ("cr", C.c_float), ("fs", C.c_float), ("alpha", C.c_float), ("gamma", C.c_float), ("beta", C.c_float),
                ("wscale", C.c_float), ("out_scale", C.c_float),
                ("out", C.c_void_p), ("energy", C.c_void_p), ("sumsq", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class DnEikonalArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("bc", DnDirichlet * 2),
                ("f", C.c_void_p), ("f_gp", C.c_void_p), ("f_batched", C.c_int32), ("f_value", C.c_float),
                ("tau", C.c_float), ("sq", C.c_float), ("wscale", C.c_float), ("vjp", C.c_int32),
                ("cot", C.c_void_p), ("in_num", C.c_void_p), ("in_den", C.c_void_p),
                ("out", C.c_void_p), ("sumsq", C.c_void_p), ("norm", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class DnCoefGradArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("v", C.c_void_p), ("bc", DnDirichlet * 2),
                ("a_nu", C.c_float), ("a_f", C.c_float), ("wscale", C.c_float),
                ("in_scale", C.c_void_p), ("g_nu", C.c_void_p), ("g_f", C.c_void_p)]


class DnPoissonDiagArgs(C.Structure):
    _fields_ = [("nu", C.c_void_p), ("nu_batched", C.c_int32), ("bc", DnDirichlet * 2),
                ("wscale", C.c_float), ("unit", C.c_int32), ("dinv", C.c_void_p)]


class DnCgState(C.Structure):
    _fields_ = [("rz", C.c_double), ("rr", C.c_double), ("rr0", C.c_double), ("pq", C.c_double),
                ("alpha", C.c_float), ("beta", C.c_float),
                ("active", C.c_int32), ("iterations", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class DnPoissonCgArgs(C.Structure):
    _fields_ = [("phase", C.c_int32), ("batch", C.c_int32), ("n", C.c_int64),
                ("x", C.c_void_p), ("r", C.c_void_p), ("p", C.c_void_p), ("q", C.c_void_p), ("dinv", C.c_void_p),
                ("dinv_batched", C.c_int32), ("tol", C.c_float), ("atol", C.c_float),
                ("state", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


CG_INIT, CG_DOT, CG_UPDATE, CG_DIRECTION = 0, 1, 2, 3
CG_BREAKDOWN = 1


class DnPoissonPcgArgs(C.Structure):
    _fields_ = [("phase", C.c_int32), ("batch", C.c_int32), ("n", C.c_int64),
                ("x", C.c_void_p), ("r", C.c_void_p), ("p", C.c_void_p), ("q", C.c_void_p), ("z", C.c_void_p),
                ("tol", C.c_float), ("atol", C.c_float),
                ("state", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


PCG_RESID0, PCG_UPDATE, PCG_RZ, PCG_DIRECTION = 0, 1, 2, 3


class DnPoissonMgArgs(C.Structure):
    _fields_ = [("op", C.c_int32), ("nsd", C.c_int32), ("batch", C.c_int32), ("fine", C.c_int32 * 3), ("coarse", C.c_int32 * 3),
                ("x", C.c_void_p), ("b", C.c_void_p), ("q", C.c_void_p), ("dinv", C.c_void_p), ("dinv_batched", C.c_int32),
                ("c", C.c_void_p), ("mask", C.c_void_p), ("mask_batched", C.c_int32), ("omega", C.c_float)]


MG_RESTRICT, MG_PROLONG, MG_SMOOTH, MG_SMOOTH0 = 0, 1, 2, 3


class DnMgParent(C.Structure):
    _fields_ = [("j", C.c_int32), ("w0", C.c_float), ("w1", C.c_float), ("pad", C.c_int32)]


class DnMgChildren(C.Structure):
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("pad", C.c_int32 * 2), ("w", C.c_float * 4)]


class DnPoissonMgTransferArgs(C.Structure):
    _fields_ = [("op", C.c_int32), ("nsd", C.c_int32), ("batch", C.c_int32), ("fine", C.c_int32 * 3), ("coarse", C.c_int32 * 3),
                ("x", C.c_void_p), ("b", C.c_void_p), ("q", C.c_void_p), ("c", C.c_void_p), ("mask", C.c_void_p),
                ("mask_batched", C.c_int32), ("parents", C.c_void_p * 3), ("children", C.c_void_p * 3)]


class DnFdmPoissonArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("ny", C.c_int32), ("nx", C.c_int32),
                ("u", C.c_void_p), ("nu", C.c_void_p), ("f", C.c_void_p), ("nu_batched", C.c_int32), ("f_batched", C.c_int32),
                ("nu_value", C.c_float), ("f_value", C.c_float), ("fs", C.c_float),
                ("bc", DnDirichlet * 2),
                ("kx", C.c_float * 9), ("ky", C.c_float * 9), ("kxx", C.c_float * 9), ("kyy", C.c_float * 9),
                ("out_scale", C.c_float), ("nbc_scale", C.c_float),
                ("in_scale", C.c_void_p), ("res", C.c_void_p), ("sums", C.c_void_p), ("grad", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class DnPointsArgs(C.Structure):
    _fields_ = [("u", C.c_void_p), ("elem", C.c_void_p), ("xi", C.c_void_p), ("offsets", C.c_void_p), ("npts", C.c_int64),
                ("dscale", C.c_float * 3), ("kind", C.c_int32), ("penalty", C.c_int32),
                ("target", C.c_void_p), ("target_value", C.c_float), ("normals", C.c_void_p), ("w_val", C.c_float), ("w_nrm", C.c_float),
                ("values", C.c_void_p), ("pgrads", C.c_void_p), ("cot", C.c_void_p), ("sums", C.c_void_p),
                ("gscale_dev", C.c_void_p), ("gscale", C.c_float), ("grad", C.c_void_p), ("accumulate", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


POINTS_NONE, POINTS_DOT, POINTS_MATCH = 0, 1, 2


class DnConvK4s2Kernel(C.Structure):
    _fields_ = [("gen", C.c_int32), ("targ", C.c_int32 * 3), ("nz", C.c_int32), ("per_slice", C.c_int32), ("sum_kernel", C.c_int32)]


CONV_DOWN, CONV_UP, CONV_WRW = 0, 1, 2


class DnPoissonKernel(C.Structure):
    _fields_ = [("family", C.c_int32), ("tile", C.c_int32 * 2), ("E", C.c_int32), ("R", C.c_int32), ("W", C.c_int32), ("ua", C.c_int32),
                ("chunks", C.c_int32), ("tiles", C.c_int32), ("strips", C.c_int32), ("launched_strips", C.c_int32),
                ("vec", C.c_int32), ("allow_e4", C.c_int32), ("compact", C.c_int32),
                ("launched", C.c_int64), ("stride", C.c_int64), ("workspace_bytes", C.c_int64)]


# dn_poisson_kernel.family (DN_POISSON_*)
POISSON_FAMILIES = {1: "2d_q1_cf", 2: "2d_q1_rule", 3: "2d_q23", 4: "3d_q1_n1", 5: "3d_q1_t16", 6: "3d_q1_generic", 7: "3d_q1_n2", 8: "3d_q1_cfz",
                    9: "3d_q23"}

I32x3 = C.c_int32 * 3

# name -> (restype, argtypes); must list every symbol of include/diffnet_hip.h
SYMBOLS = {
    "dn_abi_version": (C.c_int, []),
    "dn_build_info": (C.c_char_p, []),
    "dn_config_set": (C.c_int, [C.c_char_p, C.c_char_p]),
    "dn_config_get": (C.c_char_p, [C.c_char_p]),
    "dn_probe_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "dn_probe_march": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dn_probe_tile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dn_poisson_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_poisson_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnPoissonArgs), C.c_void_p]),
    "dn_poisson_finish_sums": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnPoissonArgs), C.c_void_p]),
    "dn_poisson_query": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnPoissonArgs), C.POINTER(DnPoissonKernel)]),
    "dn_workspace_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dn_gauss_pt_eval_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, I32x3, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_void_p]),
    "dn_gauss_pt_eval_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, I32x3, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_void_p]),
    "dn_assemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, I32x3, C.c_int32, C.c_int32, C.c_int32,
                              C.c_void_p]),
    "dn_assemble_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, I32x3, C.c_int32, C.c_int32,
                                  C.c_void_p]),
    "dn_fdm_stencil_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                     C.c_float, C.c_float, C.c_void_p]),
    "dn_fdm_stencil_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                     C.c_float, C.c_float, C.c_void_p]),
    "dn_fdm_fused_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                   C.c_float, C.c_float, C.c_void_p]),
    "dn_fdm_fused_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                   C.c_float, C.c_float, C.c_void_p]),
    "dn_fsdt_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_fsdt_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnFsdtArgs), C.c_void_p]),
    "dn_stokes_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_stokes_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnStokesArgs), C.c_void_p]),
    "dn_ns_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_ns_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnNsArgs), C.c_void_p]),
    "dn_transport_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_transport_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnTransportArgs), C.c_void_p]),
    "dn_strongform_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_strongform_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnStrongformArgs), C.c_void_p]),
    "dn_fosls_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_fosls_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnFoslsArgs), C.c_void_p]),
    "dn_helmholtz_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_helmholtz_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnHelmholtzArgs), C.c_void_p]),
    "dn_eikonal_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_eikonal_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnEikonalArgs), C.c_void_p]),
    "dn_eikonal3d_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_eikonal3d_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnEikonalArgs), C.c_void_p]),
    "dn_poisson_coef_grad": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnCoefGradArgs), C.c_void_p]),
    "dn_poisson_diag": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnPoissonDiagArgs), C.c_void_p]),
    "dn_poisson_cg_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "dn_poisson_cg": (C.c_int, [C.POINTER(DnPoissonCgArgs), C.c_void_p]),
    "dn_poisson_pcg": (C.c_int, [C.POINTER(DnPoissonPcgArgs), C.c_void_p]),
    "dn_poisson_mg": (C.c_int, [C.POINTER(DnPoissonMgArgs), C.c_void_p]),
    "dn_poisson_mg_transfer": (C.c_int, [C.POINTER(DnPoissonMgTransferArgs), C.c_void_p]),
    "dn_fdm_poisson_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "dn_fdm_poisson_apply": (C.c_int, [C.POINTER(DnFdmPoissonArgs), C.c_void_p]),
    "dn_points_workspace_bytes": (C.c_int64, [C.POINTER(DnMesh)]),
    "dn_points_apply": (C.c_int, [C.POINTER(DnMesh), C.POINTER(DnPointsArgs), C.c_void_p]),
    "dn_upconv_out_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "dn_upconv_out_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                    C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_upconv_out_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_upconv3d_out_workspace_bytes": (C.c_int64, [C.c_int64] * 5),
    "dn_upconv3d_out_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                      C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_upconv3d_out_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_conv3d_k4s2_wrw_workspace_bytes": (C.c_int64, [C.c_int64] * 6),
    "dn_conv3d_k4s2_wrw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_conv2d_k4s2_down": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int64] * 5 + [C.c_void_p]),
    "dn_conv2d_k4s2_up": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int64] * 5 + [C.c_void_p]),
    "dn_conv2d_k4s2_wrw_workspace_bytes": (C.c_int64, [C.c_int64] * 5),
    "dn_conv2d_k4s2_wrw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int64] * 5 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_conv3d_k4s2_down": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int64] * 6 + [C.c_void_p]),
    "dn_conv3d_k4s2_up": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int64] * 6 + [C.c_void_p]),
    "dn_conv3d_k4s2_workspace_bytes": (C.c_int64, [C.c_int32] + [C.c_int64] * 6),
    "dn_conv3d_k4s2_down_ws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int64] * 6 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_conv3d_k4s2_up_ws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int64] * 6 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_conv2d_k4s2_query": (C.c_int, [C.c_int32] + [C.c_int64] * 5 + [C.POINTER(DnConvK4s2Kernel)]),
    "dn_conv3d_k4s2_query": (C.c_int, [C.c_int32] + [C.c_int64] * 6 + [C.c_int32, C.POINTER(DnConvK4s2Kernel)]),
    "dn_conv2d_valid_fwd": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] * 6 + [C.c_void_p]),
    "dn_conv2d_valid_bwd_data": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 6 + [C.c_void_p]),
    "dn_conv2d_valid_bwd_weight": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] * 6 + [C.c_void_p]),
    "dn_instnorm_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "dn_instnorm_act_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_float,
                                      C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_instnorm_act_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float,
                                      C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "dn_pack_mask_bits": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "dn_unpack_mask_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "dn_winding_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_void_p]),
    "dn_winding_field_tile": (C.c_int, [C.c_int32, C.c_int64]),
    "dn_winding_field": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                   C.c_int32, C.c_void_p]),
    "dn_winding_field_vjp_slices": (C.c_int, [C.c_int32, C.c_int32, C.c_int64]),
    "dn_winding_field_vjp_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "dn_winding_field_vjp": (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_float, C.c_int32, C.c_void_p]),
}

_LIB = None


class DiffNetHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raises DiffNetHipError when the library is unusable."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise DiffNetHipError(
            f"{LIB_PATH} is missing: build it with `python -m diffnet_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the FEM hot path.")
    try:
        h = C.CDLL(LIB_PATH)
    except OSError as e:   # pragma: no cover - depends on the box
        raise DiffNetHipError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            raise DiffNetHipError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    v = h.dn_abi_version()
    if v != ABI_VERSION:
        raise DiffNetHipError(f"ABI mismatch: library {v}, binding {ABI_VERSION}")
    _LIB = h
    return h


_HIP = None


def hip_runtime():
    """ctypes handle of the HIP runtime torch runs on (the instance mapped into this process), for the few calls torch does not expose
    with the flags needed: events without the system-scope fence of a default event (1.8 us per record, tools/event_cost.py)."""
    global _HIP
    if _HIP is None:
        path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), None)
        if path is None:
            raise DiffNetHipError("the HIP runtime is not loaded in this process (no GPU build of torch?)")
        h = C.CDLL(path)
        h.hipEventCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        h.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        h.hipEventSynchronize.argtypes = [C.c_void_p]
        h.hipEventDestroy.argtypes = [C.c_void_p]
        _HIP = h
    return _HIP


def new_event():
    """A HIP event for stream ordering only: hipEventDisableTiming | hipEventDisableSystemFence."""
    e = C.c_void_p()
    rc = hip_runtime().hipEventCreateWithFlags(C.byref(e), C.c_uint(0x2 | 0x20000000))
    if rc != 0:
        raise DiffNetHipError(f"hipEventCreateWithFlags: hipError_t {rc}")
    return e


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        if rc == -4:
            raise DiffNetHipError(f"{what}: DN_E_HANDOVER (a chained-strip launch ran a bounded LDS hand-over poll to its limit: its results are NaN)")
        raise DiffNetHipError(f"{what}: {DN_E.get(rc, rc)} (argument not supported by the HIP kernels)")
    raise DiffNetHipError(f"{what}: hipError_t {rc}")


# Python-side mirror of the switches (the library reads DN_<KEY> once at load, then only dn_config_set changes them): lets host code
# that is traced by torch.compile look a switch up without a foreign call
CONFIG_MIRROR = {k[3:]: v for k, v in os.environ.items() if k.startswith("DN_")}


def config_set(key, value):
    """Set a tuning / A-B switch of the library (include/diffnet_hip.h: dn_config_set); "" or None clears it."""
    rc = lib().dn_config_set(key.encode(), (value or "").encode())
    if rc != 0:
        raise DiffNetHipError(f"dn_config_set: unknown switch {key!r} or value too long")
    CONFIG_MIRROR[key] = value or ""
    import sys
    ops = sys.modules.get(__package__ + ".ops")
    if ops is not None:
        ops.call_cache_clear()      # launch plans (and with them workspace sizes) may have changed


def config_get(key):
    v = lib().dn_config_get(key.encode())
    if v is None:
        raise DiffNetHipError(f"dn_config_get: unknown switch {key!r}")
    return v.decode()
