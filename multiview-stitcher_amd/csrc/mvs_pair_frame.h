// mvs_pair_frame.h -- internal, host side: what the entry points that reduce the sample pairs of a fixed and a moving tile over their
// overlap grid share (mvs_pair_moments, mvs_intensity_pair_moments, mvs_block_match): their common refusals, as two functions so that
// each entry keeps the order of its own between them, and the frame of the entry point after its refusals.  The argument structs stay
// in their files; the frame fills what they have in common by name, so no member moves (DESIGN section 3.17 on what 4 bytes cost).
#pragma once
#include "mvs_internal.h"
#include "mvs_fuse_dev.h"
#include <cstring>

// ndim and the halfspace count; the entry's own counts follow
inline int mvs_pair_check_counts(MvsContext* c0, const char* what, int ndim, const double* halfspaces, int n_halfspaces) {
    if (ndim != 2 && ndim != 3) return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: ndim must be 2 or 3", what);
    if (n_halfspaces < 0 || n_halfspaces > MVS_PAIR_MAX_HALFSPACES || (n_halfspaces > 0 && !halfspaces))
        return mvs_fail(c0, MVS_ERR_INVALID_ARG, "%s: n_halfspaces must be 0..%d (with their equations)", what, MVS_PAIR_MAX_HALFSPACES);
    return MVS_OK;
}

// both views, then their common dtype; the entry's per-record checks follow
inline int mvs_pair_check_views(MvsContext* c0, const char* what, const mvs_view_t* fixed, const mvs_view_t* moving, int ndim) {
    int rc = mvs_check_tile_view(c0, what, fixed, ndim);
    if (!rc) rc = mvs_check_tile_view(c0, what, moving, ndim);
    if (!rc && fixed->dtype != moving->dtype)
        rc = mvs_fail(c0, MVS_ERR_UNSUPPORTED, "%s: the views must share one dtype (%d and %d given)", what, fixed->dtype, moving->dtype);
    return rc;
}

// One entry point after its refusals: the context, both tiles staged into P.fixed and P.moving (scratch slot 0), the halfspaces in
// P.hs / P.n_hs, `prepare(c, &host, &dev)` for the entry's scratch slots 1 and 2, its mailbox and its table uploads, the timed
// `launch(tag, stream)` with tag of the tiles' type, `fold(stream, dev)`, the second launch of the entries that have one, and the
// out_bytes of result into `out`.  prepare leaves in *dev where the launches put them: the mailbox, with its CPU side in *host
// (read after the wait), or scratch slot 1 (*host stays NULL: downloaded).
template <typename Args, typename Prepare, typename Launch, typename Fold>
int mvs_pair_frame(int device, const mvs_view_t* fixed, const mvs_view_t* moving, int ndim, const double* halfspaces, int n_halfspaces, Args& P,
                   double* out, size_t out_bytes, Prepare&& prepare, Launch&& launch, Fold&& fold) {
    MvsContext* c;
    int rc = mvs_check_ready(device, &c);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    MVS_HIP_TRY(c, hipSetDevice(mvs_hip_device(device)));

    const mvs_view_t* both[2] = {fixed, moving};
    DevView* dv[2] = {&P.fixed, &P.moving};
    rc = mvs_stage_tile_views(c, both, 2, ndim, nullptr, dv);
    if (rc) return rc;
    if (n_halfspaces) memcpy(P.hs, halfspaces, sizeof(double) * 4 * n_halfspaces);
    P.n_hs = n_halfspaces;
    void *host = nullptr, *dev = nullptr;
    rc = prepare(c, &host, &dev);
    if (rc) return rc;

    MVS_HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    mvs_dispatch_dtype(fixed->dtype, [&](auto tag) { launch(tag, c->stream); });
    MVS_HIP_TRY(c, hipGetLastError());
    fold(c->stream, dev);
    MVS_HIP_TRY(c, hipGetLastError());
    MVS_HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->timing_valid = true;
    if (!host) MVS_HIP_TRY(c, hipMemcpyAsync(out, dev, out_bytes, hipMemcpyDeviceToHost, c->stream));
    MVS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (host) memcpy(out, host, out_bytes);
    return MVS_OK;
}
