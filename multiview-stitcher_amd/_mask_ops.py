"""Thin array-level wrappers of the sample-mask entry points of libmvs_hip.so (mvs_tile_histogram, mvs_mask_threshold,
mvs_label_fuse, mvs_label_contacts); the limits are checked here first, so that a refusal needs no device."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, is_device_array
from ._operands import dense_operand, fill_view_geometry, result_array, shape3, tile_view, view_data, written


def check_n_bins(n_bins):
    n_bins = int(n_bins)
    if not 1 <= n_bins <= _lib.MVS_HIST_MAX_BINS:
        raise ValueError(f"n_bins must be 1..{_lib.MVS_HIST_MAX_BINS}, not {n_bins}")
    return n_bins


def check_radius(radius, ndim):
    """``radius`` (one int or one per axis) as ``ndim`` ints in 0..MVS_MASK_MAX_DILATE."""
    radius = [int(radius)] * ndim if isinstance(radius, (int, np.integer)) else [int(r) for r in radius]
    if len(radius) != ndim:
        raise ValueError(f"expected one dilation radius or {ndim}, got {len(radius)}")
    if min(radius) < 0 or max(radius) > _lib.MVS_MASK_MAX_DILATE:
        raise ValueError(f"a dilation radius must be 0..{_lib.MVS_MASK_MAX_DILATE}, not {radius}")
    return radius


def check_n_labels(n_labels):
    n_labels = int(n_labels)
    if not 1 <= n_labels <= _lib.MVS_LABEL_MAX:
        raise ValueError(f"the number of labels must be 1..{_lib.MVS_LABEL_MAX}, not {n_labels}")
    return n_labels


def _tile_views(tiles, device):
    """The ``mvs_view_t`` array of whole 2-D / 3-D tiles of one dtype (numpy arrays or, possibly strided, DeviceArrays) and what
    keeps their memory alive."""
    if not len(tiles):
        raise ValueError("no tiles")
    views = (_lib.mvs_view_t * len(tiles))()
    keep = []
    for i, data in enumerate(tiles):
        ndim = len(data.shape)
        if ndim not in (2, 3):
            raise ValueError("tiles are 2-D or 3-D")
        if np.dtype(data.dtype) not in _lib.DTYPE_CODES:
            raise TypeError(f"unsupported dtype {data.dtype} (uint8 / uint16 / float32)")
        views[i], kept = tile_view(data, np.eye(ndim), np.zeros(ndim), device)
        keep.append(kept)
    if len({v.dtype for v in views}) != 1:
        raise TypeError("the tiles must share one dtype")
    return views, keep


def value_range(tiles, device=0):
    """``(min, max, n)`` over the voxels of all ``tiles`` that are not NaN (mvs_tile_histogram with n_bins == 0); min and max are
    NaN when n == 0."""
    lib = _lib.init(device)
    views, keep = _tile_views(tiles, device)
    lo, hi, n = C.c_double(), C.c_double(), C.c_int64()
    _lib.check(lib.mvs_tile_histogram(device, views, len(tiles), 0, None, None, C.byref(lo), C.byref(hi), C.byref(n)), device, "mvs_tile_histogram")
    del keep
    return float(lo.value), float(hi.value), int(n.value)


def bin_edges(n_bins, lo, hi):
    """numpy's own edges of ``np.histogram(..., bins=n_bins, range=(lo, hi))``."""
    return np.histogram_bin_edges(np.empty(0, dtype=np.float64), bins=int(n_bins), range=(float(lo), float(hi)))


def histogram(tiles, n_bins, lo, hi, device=0):
    """The uint64 counts of ``np.histogram(values.astype(float64), bins=n_bins, range=(lo, hi))`` over the voxels of all ``tiles``
    together (mvs_tile_histogram); NaNs and values outside the range are left out."""
    n_bins = check_n_bins(n_bins)
    if not float(hi) > float(lo):
        raise ValueError("histogram needs lo < hi")
    lib = _lib.init(device)
    views, keep = _tile_views(tiles, device)
    edges = np.ascontiguousarray(bin_edges(n_bins, lo, hi), dtype=np.float64)
    counts = np.zeros(n_bins, dtype=np.uint64)
    _lib.check(lib.mvs_tile_histogram(device, views, len(tiles), n_bins, edges.ctypes.data_as(C.POINTER(C.c_double)),
                                      counts.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None), device, "mvs_tile_histogram")
    del keep
    return counts


def threshold_mask(tile, threshold, radius=0, device=0):
    """``(mask, n_set)``: the uint8 DeviceArray ``tile > threshold``, dilated by the flat box of ``2 radius + 1`` voxels per axis
    (``scipy.ndimage.maximum_filter(mask, size=2 r + 1, mode="constant", cval=0)``), and its number of set voxels
    (mvs_mask_threshold).  ``tile``: 2-D / 3-D uint8 / uint16 / float32; a numpy array is uploaded first."""
    ndim = len(tile.shape)
    if ndim not in (2, 3):
        raise ValueError("tiles are 2-D or 3-D")
    radius = check_radius(radius, ndim)
    if np.dtype(tile.dtype) not in _lib.DTYPE_CODES:
        raise TypeError(f"unsupported dtype {tile.dtype} (uint8 / uint16 / float32)")
    lib = _lib.init(device)
    if not is_device_array(tile):
        tile = DeviceArray.from_host(tile, device)
    view, keep = tile_view(tile, np.eye(ndim), np.zeros(ndim), device)
    out = DeviceArray.empty(tile.shape, np.uint8, device)
    n_set = C.c_int64()
    _lib.check(lib.mvs_mask_threshold(device, C.byref(view), ndim, float(threshold), _lib.i32x3(radius, ndim, 0), C.c_void_p(out.ptr), C.byref(n_set)),
               device, "mvs_mask_threshold")
    out.mark_written()
    del keep
    return out, int(n_set.value)


def check_feather_width(width, ndim):
    """``width`` (one int or one per axis) as ``ndim`` ints in 1..MVS_FEATHER_MAX_WIDTH; the one number 0 means no feather, which
    is width 1 on every axis (a step of one voxel is already the whole width)."""
    if isinstance(width, (int, np.integer)) and not isinstance(width, bool):
        width = [1 if int(width) == 0 else int(width)] * ndim
    else:
        if any(isinstance(w, bool) or not isinstance(w, (int, np.integer)) for w in width):
            raise TypeError(f"a feather width is an integer number of voxels, not {list(width)}")
        width = [int(w) for w in width]
    if len(width) != ndim:
        raise ValueError(f"expected one feather width or {ndim}, got {len(width)}")
    if min(width) < 1 or max(width) > _lib.MVS_FEATHER_MAX_WIDTH:
        raise ValueError(f"a feather width must be 1..{_lib.MVS_FEATHER_MAX_WIDTH} (or the one number 0: no feather), not {width}")
    return width


def feather(mask, width, device=0, out_on_device=False):
    """The uint8 weight tile ``rint(252 (1 - cos(pi min(t, 1))) / 2)`` of a 2-D / 3-D uint8 mask, ``t`` the distance to the mask's
    nearest zero voxel in units of ``width`` per axis (mvs_mask_feather).  ``mask``: numpy array or (possibly strided, x contiguous)
    DeviceArray; the result is a numpy array, or a DeviceArray with ``out_on_device``."""
    ndim = len(mask.shape)
    if ndim not in (2, 3):
        raise ValueError("masks are 2-D or 3-D")
    width = check_feather_width(width, ndim)
    if np.dtype(mask.dtype) != np.uint8:
        raise TypeError(f"masks are uint8, not {mask.dtype}")
    lib = _lib.init(device)
    view, keep = tile_view(mask, np.eye(ndim), np.zeros(ndim), device)
    out, ptr, mem = result_array(mask.shape, np.uint8, out_on_device, device)
    _lib.check(lib.mvs_mask_feather(device, C.byref(view), ndim, _lib.i32x3(width, ndim, 1), C.c_void_p(ptr), mem), device, "mvs_mask_feather")
    del keep
    return written(out)


def fuse_labels(masks, matrices, offsets, out_shape, device=0, out_on_device=False):
    """The int32 label volume of shape ``out_shape``: per voxel the minimum over the views ``i`` that cover it at order 0 of
    ``masks[i] ? i + 1 : 0``, and 0 where none does (mvs_label_fuse).  ``masks``: uint8 arrays (numpy or DeviceArray);
    ``matrices[i]``, ``offsets[i]`` map an index of the output grid to a pixel of view ``i`` (``transformation.get_pixel_affines``)."""
    lib = _lib.init(device)
    ndim = len(out_shape)
    if ndim not in (2, 3) or any(len(m.shape) != ndim for m in masks):
        raise ValueError("fuse_labels needs 2-D or 3-D masks and an output shape of the same rank")
    views = (_lib.mvs_view_t * len(masks))()
    keep = []
    for view, mask, matrix, offset in zip(views, masks, matrices, offsets):
        if np.dtype(mask.dtype) != np.uint8:
            raise TypeError(f"masks are uint8, not {mask.dtype}")
        ptr, s3, st3, mem, kept = view_data(mask, device)
        fill_view_geometry(view, ptr, _lib.MVS_U8, mem, s3, st3, matrix, offset)
        keep.append(kept)
    out, ptr, mem = result_array(out_shape, np.int32, out_on_device, device)
    _lib.check(lib.mvs_label_fuse(device, views, len(masks), ndim, _lib.i64x3(shape3(out_shape)), C.c_void_p(ptr), mem), device, "mvs_label_fuse")
    del keep
    return written(out)


def label_contacts(labels, n_labels, connectivity=None, device=0):
    """The ``(n_labels, n_labels)`` uint64 matrix of contact counts of a 2-D / 3-D int32 label volume (mvs_label_contacts):
    ``C[a - 1, b - 1]``, ``a < b``, counts the voxel pairs ``(p, p + o)`` with the labels ``{a, b}``, ``o`` over the half
    neighbourhood in which up to ``connectivity`` axes differ (default: all).  ``labels``: numpy array (uploaded) or contiguous
    DeviceArray."""
    n_labels = check_n_labels(n_labels)
    ndim = len(labels.shape)
    if ndim not in (2, 3):
        raise ValueError("label volumes are 2-D or 3-D")
    connectivity = ndim if connectivity is None else int(connectivity)
    if not 1 <= connectivity <= ndim:
        raise ValueError(f"connectivity must be 1..{ndim}")
    if np.dtype(labels.dtype) != np.int32:
        raise TypeError(f"label volumes are int32, not {labels.dtype}")
    lib = _lib.init(device)
    if not is_device_array(labels):
        host = np.ascontiguousarray(labels)
        labels = DeviceArray.empty(host.shape, np.int32, device)
        _lib.check(lib.mvs_memcpy_h2d(device, labels.ptr, host.ctypes.data, host.nbytes), device, "h2d")
    ptr, _, keep = dense_operand(labels, (np.int32,), device, "mvs_label_contacts")
    counts = np.zeros((n_labels, n_labels), dtype=np.uint64)
    _lib.check(lib.mvs_label_contacts(device, C.c_void_p(ptr), ndim, _lib.i64x3(shape3(labels.shape)), n_labels, connectivity,
                                      counts.ctypes.data_as(C.POINTER(C.c_uint64))), device, "mvs_label_contacts")
    return counts
