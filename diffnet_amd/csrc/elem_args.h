// Host side of what the element operators' argument structs (dn_strongform_args ... dn_eikonal_args) and their kernel parameters (those
// derived from Elem2dParams, and Ek3Params) have in common by member name, in any dimension: the forcing, the conditions, the workspace.
#pragma once
#include "dn_reduce.h"

namespace dn {
// After the operator's own DN_E_BADARG checks: the forcing and the two conditions
template <class Args>
static int elem_check_conditions(const Args* a) {
    if (a->f && a->f_gp) return DN_E_BADARG;
    if (a->f_batched & ~1) return DN_E_BADARG;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        if (d.mask_kind == DN_MASK_BITS || d.mask_kind == DN_MASK_BOX) return DN_E_UNSUPPORTED;     // expand them: dn_unpack_mask_bits
        if (d.mask_kind != DN_MASK_F32 && d.mask_kind != DN_MASK_U8) return DN_E_BADARG;
        if ((d.mask_batched | d.field_batched) & ~1) return DN_E_BADARG;
        if (d.field && !d.mask) return DN_E_BADARG;                           // a value field without its mask
    }
    return 0;
}

template <class Params, class Args>
static void elem_fill_conditions(Params& pp, const Args* a) {
    pp.f = a->f; pp.fgp = a->f_gp; pp.f_batched = a->f_batched;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        pp.mask[k] = d.mask;
        pp.mask_kind[k] = !d.mask ? 0 : (d.mask_kind == DN_MASK_U8 ? 1 : 2);
        pp.mask_batched[k] = d.mask_batched;
        pp.bcf[k] = d.field;
        pp.bcf_batched[k] = d.field_batched;
        pp.bcv[k] = d.value;
    }
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER) : nullptr;
}
}  // namespace dn
