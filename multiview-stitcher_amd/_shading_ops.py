"""Thin array-level wrappers of the shading correction entry points of libmvs_hip.so (mvs_stack_quantiles, mvs_plane_apply) and the
host form of the rank rule they share with ``intensity.py`` and the oracle."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._intensity_ops import apply_to_tile
from ._operands import dense_operand, fill_view_geometry, shape3, view_data


# ---- the rank rule (include/mvs_hip.h) --------------------------------------------------------------------------------------------
def rank_of(n, q):
    """Ascending 0-based rank of quantile ``q`` among ``n >= 1`` samples: ``floor((n - 1) * q)`` in float64 -- numpy's
    ``quantile(..., method="lower")``.  ``n`` may be an array; where ``n == 0`` the rank is 0."""
    n = np.asarray(n, dtype=np.int64)
    return np.floor(np.maximum(n - 1, 0).astype(np.float64) * float(q)).astype(np.int64)


def every_kth_plane(data, k):
    """Planes 0, k, 2k, ... of a 3-D tile, by stride (no copy): a numpy view or a ``DeviceArray`` window."""
    from .device import DeviceArray, is_device_array

    k = int(k)
    if k < 1:
        raise ValueError("plane_step must be at least 1")
    if k == 1 or len(data.shape) != 3:
        return data
    if not is_device_array(data):
        return data[::k]
    n = (data.shape[0] + k - 1) // k
    return DeviceArray(data._buf, data.ptr, (n,) + tuple(data.shape[1:]), (data.strides[0] * k,) + tuple(data.strides[1:]), data.dtype,
                       data.device, pending=data._pending)


def _stack_view(tile, device):
    """The mvs_view_t of one tile of a stack: a ``DeviceArray`` or a numpy array whose rows are contiguous is read in place, with its
    own plane and row strides; any other host array is copied."""
    from .device import is_device_array

    view = _lib.mvs_view_t()
    if is_device_array(tile):
        ptr, s3, st3, mem, keep = view_data(tile, device)
    else:
        keep = np.asarray(tile)
        if keep.dtype not in _lib.DTYPE_CODES:
            raise TypeError(f"unsupported dtype {keep.dtype} (uint8 / uint16 / float32)")
        item = keep.dtype.itemsize
        if any(s % item or s < 0 for s in keep.strides) or (keep.shape[-1] > 1 and keep.strides[-1] != item):
            keep = np.ascontiguousarray(keep)
        s3 = shape3(keep.shape)
        st = [0] * (3 - keep.ndim) + [s // item for s in keep.strides]
        dense = [s3[1] * s3[2], s3[2], 1]
        st3 = [d if n == 1 else s for s, d, n in zip(st, dense, s3)]          # (numpy's strides of size-1 axes are arbitrary)
        ptr, mem = keep.ctypes.data, _lib.MVS_MEM_HOST
    fill_view_geometry(view, ptr, _lib.DTYPE_CODES[np.dtype(keep.dtype)], mem, s3, st3, np.eye(3), np.zeros(3))
    return view, keep


def stack_quantiles(tiles, q, device=0):
    """Per-pixel order statistics of a stack of tiles (mvs_stack_quantiles): ``(planes float32 (n_q, H, W), counts int32 (H, W))``.

    ``tiles``: 2-D ``(H, W)`` or 3-D ``(z, H, W)`` arrays of one dtype (uint8 / uint16 / float32) and one ``(H, W)``, numpy arrays
    or ``DeviceArray`` windows (rows contiguous; plane and row strides arbitrary); ``z`` may differ per tile.  ``q``: one quantile
    or up to MVS_STACK_MAX_QUANTILES of them in [0, 1].  ``planes[j][y, x]`` is the sample of rank ``rank_of(counts[y, x], q[j])``
    among the values of pixel ``(y, x)`` over all tiles and planes, float32 NaNs left out; NaN where there is none."""
    lib = _lib.init(device)
    tiles = list(tiles)
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qs.ndim != 1 or not 1 <= len(qs) <= _lib.MVS_STACK_MAX_QUANTILES or not np.all((qs >= 0) & (qs <= 1)):
        raise ValueError(f"q: 1..{_lib.MVS_STACK_MAX_QUANTILES} quantiles in [0, 1]")
    if not 1 <= len(tiles) <= _lib.MVS_STACK_MAX_VIEWS:
        raise ValueError(f"stack_quantiles takes 1..{_lib.MVS_STACK_MAX_VIEWS} tiles")
    ndims = {len(t.shape) for t in tiles}
    if ndims - {2, 3}:
        raise ValueError("stack_quantiles needs 2-D or 3-D tiles")
    if len({tuple(t.shape[-2:]) for t in tiles}) != 1 or len({np.dtype(t.dtype) for t in tiles}) != 1:
        raise ValueError("the tiles of a stack share one (H, W) and one dtype")
    views = (_lib.mvs_view_t * len(tiles))()
    keep = []
    for i, t in enumerate(tiles):
        v, k = _stack_view(t, device)
        C.memmove(C.byref(views[i]), C.byref(v), C.sizeof(_lib.mvs_view_t))
        keep.append(k)
    h, w = (int(s) for s in tiles[0].shape[-2:])
    planes = np.empty((len(qs), h, w), dtype=np.float32)
    counts = np.empty((h, w), dtype=np.int32)
    rc = lib.mvs_stack_quantiles(device, views, len(tiles), 3 if 3 in ndims else 2, qs.ctypes.data_as(C.POINTER(C.c_double)), len(qs),
                                 planes.ctypes.data_as(C.POINTER(C.c_float)), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    _lib.check(rc, device, "mvs_stack_quantiles")
    del keep
    return planes, counts


def apply_plane(data, coeff, out=None, out_dtype=None, device=0):
    """``a(y, x) * data + b(y, x)`` for one 2-D / 3-D tile (mvs_plane_apply).  ``coeff``: float32 ``(H, W, 2)``, gain and offset
    per pixel, a numpy array or a contiguous ``DeviceArray`` (callers that correct many tiles upload it once).  ``data``, ``out``
    and ``out_dtype`` as in ``_intensity_ops.apply_map``: the result is of the data's kind, of the input's dtype (the default) or
    float32; ``out is data`` corrects a contiguous array in place."""
    lib = _lib.init(device)
    ndim = len(data.shape)
    coeff_ptr, coeff_mem, coeff = dense_operand(coeff, (np.float32,), device, "the coefficients of apply_plane", host_dtype=np.float32, error=ValueError)
    if ndim not in (2, 3) or tuple(coeff.shape) != tuple(int(s) for s in data.shape[-2:]) + (2,):
        raise ValueError("apply_plane needs a 2-D or 3-D tile and coefficients of shape (H, W, 2)")
    return apply_to_tile("mvs_plane_apply", data, out, out_dtype, device, lambda view, out_ptr, out_code, out_mem: lib.mvs_plane_apply(
        device, view, ndim, C.c_void_p(coeff_ptr), coeff_mem, out_ptr, out_code, out_mem))
