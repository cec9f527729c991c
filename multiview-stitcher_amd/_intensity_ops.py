"""Thin array-level wrappers of the intensity harmonisation entry points of libmvs_hip.so (mvs_intensity_pair_moments,
mvs_intensity_apply) and the host form of the cell rule they share with the planner and the solver of ``intensity.py``."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._metric_ops import box3, moments_in_groups, pair_call_views
from ._operands import result_array, shape3, tile_view, written


# ---- the cell rule (include/mvs_hip.h) ------------------------------------------------------------------------------------------
def cell_index(c, g, n):
    """Cell of the continuous pixel coordinate(s) ``c`` along an axis of ``n`` pixels with ``g`` cells:
    ``clamp(floor((c + 0.5) * g / n), 0, g - 1)`` in float64, the product before the quotient."""
    k = np.floor((np.asarray(c, dtype=np.float64) + 0.5) * float(g) / float(n))
    return np.clip(k, 0, g - 1).astype(np.int64)


def cell_centres(g, n):
    """Pixel coordinates of the centres of the ``g`` cells of an axis of ``n`` pixels: ``(k + 0.5) * n / g - 0.5``."""
    return (np.arange(g, dtype=np.float64) + 0.5) * float(n) / float(g) - 0.5


def axis_table(n, g):
    """What mvs_intensity_apply reads per pixel index of one axis: ``(lower cell int32[n], weight float32[n])``.  The pixel
    coordinate is clamped to the first and last cell centre; with ``u`` its position in units of the centre spacing, the lower cell
    is ``min(floor(u), g - 2)`` and the weight of the cell above it ``u - lower``, both derived in float64.  ``g == 1``: cell 0,
    weight 0."""
    if g == 1:
        return np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
    ctr = cell_centres(g, n)
    p = np.clip(np.arange(n, dtype=np.float64), ctr[0], ctr[-1])
    u = (p - ctr[0]) / (float(n) / float(g))
    lower = np.clip(np.floor(u), 0, g - 2)
    return lower.astype(np.int32), (u - lower).astype(np.float32)


def cell_pair_moments(fixed, moving, fixed_affine, moving_affine, cells_f, cells_m, records, halfspaces=None, device=0, batch=None):
    """Moments of the sample pairs of two tiles per record (mvs_intensity_pair_moments): an ``(R, 6)`` float64 array with the rows
    ``(n, mean_f, mean_m, M2_f, M2_m, C_fm)``.

    ``fixed`` / ``moving``: 2-D / 3-D tiles of one dtype, numpy arrays or ``DeviceArray`` windows; ``fixed_affine`` /
    ``moving_affine = (matrix, offset)`` map a grid index to a pixel of the tile; ``cells_f`` / ``cells_m``: cells per axis.
    ``records``: int64 array ``(R, 4, ndim)`` with the rows ``lo, n, cell_f, cell_m`` (``intensity.plan_records``).  ``halfspaces``
    as in ``_metric_ops.pair_moments``.  Records go to the device in groups of ``batch`` (default and at most
    MVS_INTENSITY_MAX_RECORDS); a record's row does not depend on its group."""
    lib = _lib.init(device)
    records = np.asarray(records, dtype=np.int64)
    ndim = len(cells_f)
    if ndim not in (2, 3) or records.ndim != 3 or records.shape[1:] != (4, ndim):
        raise ValueError("cell_pair_moments needs 2-D or 3-D cells and records of shape (R, 4, ndim)")
    batch = _lib.MVS_INTENSITY_MAX_RECORDS if batch is None else int(batch)
    if not 1 <= batch <= _lib.MVS_INTENSITY_MAX_RECORDS:
        raise ValueError(f"batch must be 1..{_lib.MVS_INTENSITY_MAX_RECORDS}")
    fview, mview, hs_ptr, n_hs, keep = pair_call_views(fixed, moving, fixed_affine, moving_affine, halfspaces, ndim, device)
    cf, cm = _lib.i32x3(cells_f, ndim, 1), _lib.i32x3(cells_m, ndim, 1)

    def call(group):
        recs = (_lib.mvs_intensity_record_t * len(group))()
        for rec, row in zip(recs, box3(group, (0, 1, 0, 0))):
            rec.lo[:], rec.n[:], rec.cell_f[:], rec.cell_m[:] = row
        res = np.zeros((len(group), _lib.MVS_PAIR_MOMENTS_LEN))
        _lib.check(lib.mvs_intensity_pair_moments(device, C.byref(fview), C.byref(mview), ndim, cf, cm, hs_ptr, n_hs, recs, len(group),
                                                  res.ctypes.data_as(C.POINTER(C.c_double))), device, "mvs_intensity_pair_moments")
        return res

    return moments_in_groups(records, batch, call)      # (`keep` lives until here)


def apply_to_tile(name, data, out, out_dtype, device, call):
    """What ``apply_map`` and ``_shading_ops.apply_plane`` share: the result is of the data's kind and of ``out_dtype`` (the input's
    dtype, the default, or float32); ``out`` (allocated when None) is a contiguous array of the data's kind and shape and of
    ``out_dtype``.  ``call(view, out_ptr, out_dtype_code, out_mem)`` runs entry point ``name`` and returns its code."""
    from .device import is_device_array

    ndim = len(data.shape)
    in_dtype = np.dtype(data.dtype)
    if in_dtype not in _lib.DTYPE_CODES:
        raise TypeError(f"unsupported dtype {in_dtype} (uint8 / uint16 / float32)")
    out_dtype = in_dtype if out_dtype is None else np.dtype(out_dtype)
    if out_dtype not in (in_dtype, np.dtype(np.float32)):
        raise TypeError(f"out_dtype must be the input's dtype or float32, not {out_dtype}")
    out, out_ptr, out_mem = result_array(data.shape, out_dtype, is_device_array(data), device, out)
    view, keep = tile_view(data, np.eye(ndim), np.zeros(ndim), device)
    _lib.check(call(C.byref(view), C.c_void_p(out_ptr), _lib.DTYPE_CODES[out_dtype], out_mem), device, name)
    del keep
    return written(out)


def apply_map(data, coeff, out=None, out_dtype=None, device=0):
    """``a(p) * data + b(p)`` for one 2-D / 3-D tile (mvs_intensity_apply).  ``coeff``: float32 ``cells + (2,)``, gain and offset
    per cell, interpolated multilinearly between the cell centres.  ``data``: numpy array or (possibly strided) ``DeviceArray``;
    the result is of the same kind, of ``out_dtype`` (the input's dtype, the default, or float32).  ``out``: where the result goes
    -- a contiguous array of the data's shape and ``out_dtype``; ``out is data`` corrects a contiguous array in place."""
    lib = _lib.init(device)
    coeff = np.ascontiguousarray(coeff, dtype=np.float32)
    ndim = coeff.ndim - 1
    if ndim not in (2, 3) or coeff.shape[-1] != 2 or len(data.shape) != ndim:
        raise ValueError("apply_map needs a 2-D or 3-D tile and coefficients of shape cells + (2,)")
    cells = coeff.shape[:-1]
    tables = np.concatenate([part.view(np.uint8) for n, g in zip(shape3(data.shape), shape3(cells)) for part in axis_table(n, g)])
    return apply_to_tile("mvs_intensity_apply", data, out, out_dtype, device, lambda view, out_ptr, out_code, out_mem: lib.mvs_intensity_apply(
        device, view, ndim, _lib.i32x3(cells, ndim, 1), coeff.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(tables.ctypes.data), out_ptr, out_code, out_mem))
