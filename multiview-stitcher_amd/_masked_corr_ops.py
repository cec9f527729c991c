"""Thin array-level wrapper of mvs_masked_corr (libmvs_hip.so) and the host pieces around it: the padded shape and its limit,
checked here first so that a refusal needs no device, and the sub-pixel parabola."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._operands import operand_pair, shape3
from .device import is_device_array

STATUS_MESSAGES = {
    _lib.MVS_MASKED_CORR_NO_ELIGIBLE_SHIFT: "no shift of the window has enough overlap and a positive variance in both crops",
    _lib.MVS_MASKED_CORR_TOO_FEW_VALID: "a crop has fewer than min_overlap valid voxels",
    _lib.MVS_MASKED_CORR_CONSTANT_CROP: "a crop is constant on its valid voxels",
}


def per_axis_shift(max_shift, shape):
    """``max_shift`` (None, one value or one per axis, in px) as the largest |shift| searched per axis: ``n - 1`` where it is
    None or larger."""
    ndim = len(shape)
    if max_shift is None:
        return [int(n) - 1 for n in shape]
    vals = [max_shift] * ndim if np.isscalar(max_shift) else list(max_shift)
    if len(vals) != ndim:
        raise ValueError(f"expected one max_shift or {ndim}, got {len(vals)}")
    if any(v < 0 for v in vals):
        raise ValueError(f"max_shift must not be negative, got {max_shift}")
    return [min(int(v), int(n) - 1) for v, n in zip(vals, shape)]


def padded_shape(shape, shifts):
    """Per axis the smallest power of two >= n + S (1 for an axis of one voxel): mvs_masked_corr_plan.h."""
    out = []
    for n, s in zip(shape, shifts):
        p = 1
        while int(n) > 1 and p < int(n) + int(s):
            p <<= 1
        out.append(p)
    return tuple(out)


def check_limit(shape, shifts):
    padded = padded_shape(shape, shifts)
    total = 1
    for p in padded:
        total *= p
    if total > _lib.MVS_MASKED_CORR_MAX_VOXELS:
        raise NotImplementedError(
            f"masked correlation of crops of shape {tuple(shape)} with shifts up to {tuple(shifts)} px needs transforms of {padded} = {total} voxels, "
            f"more than MVS_MASKED_CORR_MAX_VOXELS = {_lib.MVS_MASKED_CORR_MAX_VOXELS}: pass a smaller max_shift"
        )
    return padded


def subpixel_offset(centre, left, right, left_ok=True, right_ok=True):
    """Vertex of the parabola through ``r`` at the peak and its two neighbours along one axis, as an offset in px from the peak:
    ``0.5 (l - r) / (l - 2 c + r)``, clamped to +-0.5; 0 unless both neighbours count (inside the window and eligible), all three
    values are finite and the curvature ``l - 2 c + r`` is negative.  float64."""
    if not (left_ok and right_ok):
        return 0.0
    c, l, r = float(centre), float(left), float(right)
    if not (np.isfinite(c) and np.isfinite(l) and np.isfinite(r)):
        return 0.0
    curvature = l - 2.0 * c + r
    if not curvature < 0.0:
        return 0.0
    return float(min(max(0.5 * (l - r) / curvature, -0.5), 0.5))


def _host_mask_as_uint8(m):
    """A host mask (anything numpy turns into booleans) as uint8; None and DeviceArrays pass through."""
    if m is None or is_device_array(m):
        return m
    m = np.asarray(m)
    return m if m.dtype == np.uint8 else (m != 0).astype(np.uint8)


def masked_corr(fixed, moving, fixed_mask=None, moving_mask=None, valid_above=(None, None), overlap_ratio=0.3, min_overlap=1, shifts=None,
                device=0, want_volumes=False):
    """One mvs_masked_corr call.  ``fixed`` / ``moving``: float32 crops of one shape, both numpy arrays or both contiguous
    DeviceArrays; the masks (uint8, or anything numpy turns into booleans) both on one side as well.  ``shifts``: per axis the
    largest |shift| (``per_axis_shift``).  Returns a dict with the fields of ``mvs_masked_corr_result_t`` cut to the crop's
    rank, plus ``r`` / ``n`` window volumes of shape ``2 S + 1`` with ``want_volumes``."""
    shape = tuple(int(s) for s in fixed.shape)
    ndim = len(shape)
    if ndim not in (2, 3):
        raise ValueError("crops are 2-D or 3-D")
    if tuple(int(s) for s in moving.shape) != shape:
        raise ValueError("fixed and moving crops must have the same shape")
    if not 0.0 < float(overlap_ratio) <= 1.0:
        raise ValueError(f"overlap_ratio must be in (0, 1], not {overlap_ratio}")
    if int(min_overlap) < 1:
        raise ValueError("min_overlap must be at least 1")
    shifts = per_axis_shift(shifts, shape)
    check_limit(shape, shifts)
    for m, name in ((fixed_mask, "fixed_mask"), (moving_mask, "moving_mask")):
        if m is not None and tuple(int(s) for s in m.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(m.shape)}, the crops have {shape}")
    p0, p1, mem, keep = operand_pair(fixed, moving, (np.float32,), device, "masked correlation", host_dtype=np.float32, names="crops")
    q0, q1, mask_mem, mask_keep = operand_pair(_host_mask_as_uint8(fixed_mask), _host_mask_as_uint8(moving_mask), (np.uint8,), device,
                                               "masked correlation", names="masks")
    lib = _lib.init(device)
    opts = _lib.mvs_masked_corr_opts_t()
    opts.ndim = ndim
    opts.mem = mem
    opts.mask_mem = mask_mem
    for k, thr in enumerate(valid_above):
        opts.has_valid_above[k] = 0 if thr is None else 1
        opts.valid_above[k] = 0.0 if thr is None else float(thr)
    opts.overlap_ratio = float(overlap_ratio)
    opts.min_overlap = int(min_overlap)
    for k, s in enumerate(shape3(shifts)):
        opts.max_shift[k] = int(s) if k >= 3 - ndim else -1
    res = _lib.mvs_masked_corr_result_t()
    window = tuple(2 * s + 1 for s in shifts)
    r_vol = np.empty(window, dtype=np.float32) if want_volumes else None
    n_vol = np.empty(window, dtype=np.int32) if want_volumes else None
    _lib.check(lib.mvs_masked_corr(device, p0, p1, q0, q1, _lib.i64x3(shape3(shape)), C.byref(opts), C.byref(res),
                                   r_vol.ctypes.data if want_volumes else None, n_vol.ctypes.data if want_volumes else None),
               device, "mvs_masked_corr")
    del keep, mask_keep
    k = 3 - ndim
    out = {
        "status": int(res.status),
        "peak": [int(v) for v in res.peak][k:],
        "r": float(res.r),
        "n_peak": int(res.n_peak),
        "n_max": int(res.n_max),
        "n_valid": (int(res.n_valid[0]), int(res.n_valid[1])),
        "neighbour_r": [float(v) for v in res.neighbour_r][2 * k:],
        "neighbour_ok": [bool(v) for v in res.neighbour_ok][2 * k:],
        "padded_shape": tuple(int(v) for v in res.padded)[k:],
        "max_shift": tuple(int(v) for v in res.max_shift)[k:],
    }
    if want_volumes:
        out["r_volume"], out["n_volume"] = r_vol, n_vol
    return out
