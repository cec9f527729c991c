// mvs_affine_walk.h -- host side of the entry points that launch a walk of mvs_affine_walk_dev.h (mvs_affine_normal_eq,
// mvs_affine_joint_hist, mvs_affine_mi_gradient): the argument checks and the launch geometry they share.
#pragma once
#include "mvs_affine_walk_dev.h"
#include "mvs_internal.h"

// The checks that need no device.  out0 / out1: the entry's result (or table) pointers; `who` names it in the messages.
static inline int affine_check_args(MvsContext* c0, const char* who, const void* fixed, const void* moving, int32_t mem, int32_t ndim,
                                    const int64_t* shape, const double* matrix, const double* offset, const void* out0, const void* out1) {
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", who);
    if (!fixed || !moving || !shape || !matrix || !offset || !out0 || !out1) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (mem != MVS_MEM_HOST && mem != MVS_MEM_DEVICE) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: bad mem", who);
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 1 || (k < 3 - ndim && shape[k] != 1))
            return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: shape must be positive (and 1 along z in 2D)", who);
    for (int k = 0; k < 3; ++k)
        if (shape[k] > (1 << 24)) return mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: axis longer than 2^24", who);
    return MVS_OK;
}

// Fills the walk of a checked call, counts its blocks and stages both crops (scratch slots 4 and 5).  c is the locked context.
static inline int affine_walk_setup(MvsContext* c, const char* who, const float* fixed, const float* moving, int32_t mem, const int64_t shape[3],
                                    const double matrix[9], const double offset[3], mvs_aw::Walk* W, long long* nblocks) {
    *nblocks = mvs_aw::set_geometry(W, shape, matrix, offset);
    if (*nblocks > 0x7fffffffll) return mvs_fail(c, MVS_ERR_UNSUPPORTED, "%s: crop too large", who);
    const long long n = (long long)shape[0] * shape[1] * shape[2];
    float *dF, *dM;
    int rc = mvs_stage_float_volume(c, fixed, mem, n, 4, &dF);
    if (rc) return rc;
    rc = mvs_stage_float_volume(c, moving, mem, n, 5, &dM);
    if (rc) return rc;
    W->fixed = dF;
    W->moving = dM;
    return MVS_OK;
}
