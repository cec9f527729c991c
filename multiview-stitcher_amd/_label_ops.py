"""Thin array-level wrappers of the label entry points of libmvs_hip.so (mvs_label_counts, mvs_label_pair_overlaps,
mvs_label_tiles_fuse, mvs_label_components).  Label tiles are int32 by contract: a host tile of another integer dtype is converted
here, a device tile must be int32 already.  The capacities the entries ask for are the callers' business nowhere else: the retries
live here.  ``label_components`` alone takes IMAGE tiles (uint8 / uint16 / float32) and makes label tiles of them."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, is_device_array
from ._operands import fill_view_geometry, result_array, shape3, view_data, written

INT32_MAX = 2**31 - 1
_TILE_DTYPES = (np.dtype(np.int32),) + tuple(_lib.DTYPE_CODES)      # label tiles, and the image tiles of label_components
COUNT_CAPACITY = 1 << 16        # first try of mvs_label_counts: labels 0 .. 65 535
PAIR_CAPACITY = 1 << 16         # first try of mvs_label_pair_overlaps: a table of 2^17 slots (2 MiB)


def as_label_tile(data, who="label tile"):
    """A label tile as the entries take it: a 2-D / 3-D int32 array.  Host arrays of any integer dtype are converted (a value above
    2^31 - 1 raises ValueError; negative values are background and become -1 where they do not fit); a DeviceArray must be int32
    with contiguous rows (strided windows are fine)."""
    if is_device_array(data):
        if np.dtype(data.dtype) != np.int32:
            raise TypeError(f"{who}: device label tiles are int32, not {data.dtype}")
        if len(data.shape) not in (2, 3):
            raise ValueError(f"{who}: label tiles are 2-D or 3-D")
        if data.strides[-1] != 1 and data.shape[-1] > 1:
            raise TypeError(f"{who}: device label tiles need contiguous rows (stride 1 along x)")
        return data
    data = np.asarray(data)
    if data.ndim not in (2, 3):
        raise ValueError(f"{who}: label tiles are 2-D or 3-D")
    if data.dtype == np.bool_ or not np.issubdtype(data.dtype, np.integer):
        raise TypeError(f"{who}: label tiles are integers, not {data.dtype}")
    if data.dtype != np.int32:
        if data.size and int(data.max()) > INT32_MAX:
            raise ValueError(f"{who}: label {int(data.max())} exceeds 2^31 - 1")
        if np.issubdtype(data.dtype, np.signedinteger) and data.dtype.itemsize > 4:
            data = np.maximum(data, -1)
        data = data.astype(np.int32)
    return np.ascontiguousarray(data)


def to_device(tile, device=0):
    """A host label tile as a resident int32 DeviceArray."""
    host = as_label_tile(tile)
    lib = _lib.init(device)
    dev = DeviceArray.empty(host.shape, np.int32, device)
    _lib.check(lib.mvs_memcpy_h2d(device, dev.ptr, host.ctypes.data, host.nbytes), device, "h2d")
    dev.mark_written()
    return dev


def label_view(tile, matrix, offset, device):
    """``(mvs_view_t, array to keep alive)`` of a label tile from ``as_label_tile``; ``matrix`` / ``offset`` (None: the identity)
    map an index of the walked grid to a pixel of the tile.  The dtype field is not read by the label entries."""
    ndim = len(tile.shape)
    ptr, s3, st3, mem, keep = view_data(tile, device, allow=_TILE_DTYPES)
    st3[2] = 1          # (the stride of an axis of one voxel is arbitrary)
    view = _lib.mvs_view_t()
    fill_view_geometry(view, ptr, 0, mem, s3, st3, np.eye(ndim) if matrix is None else np.asarray(matrix, dtype=np.float64),
                       np.zeros(ndim) if offset is None else np.asarray(offset, dtype=np.float64))
    return view, keep


def label_counts(tile, device=0, capacity=None):
    """The uint64 array ``n[l]``, ``l = 0 .. max label``, of the voxels of ``tile`` with label ``l`` (mvs_label_counts); negative
    labels count as 0.  ``capacity``: the first array size to try; the call is repeated once with ``max + 1`` when a label does not
    fit."""
    tile = as_label_tile(tile)
    lib = _lib.init(device)
    view, keep = label_view(tile, None, None, device)
    capacity = COUNT_CAPACITY if capacity is None else int(capacity)
    if capacity < 1:
        raise ValueError("capacity must be >= 1")
    while True:
        counts = np.zeros(capacity, dtype=np.uint64)
        mx = C.c_int64()
        _lib.check(lib.mvs_label_counts(device, C.byref(view), len(tile.shape), capacity, counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(mx)),
                   device, "mvs_label_counts")
        if mx.value < capacity:
            del keep
            return counts[:mx.value + 1].copy()
        capacity = int(mx.value) + 1


def pair_overlaps(tile_a, tile_b, matrix, offset, box_lo, box_n, device=0, capacity=None):
    """The co-occurrence table of the directed pair ``(a, b)`` as ``(la, lb, n)``, int32 / int32 / uint64, sorted by ``(la, lb)``
    (mvs_label_pair_overlaps).  ``matrix`` / ``offset`` map a pixel index of ``a`` to a pixel coordinate of ``b``; ``box_lo`` /
    ``box_n``: the box of ``a`` that is walked (empty: an empty table, no call).  ``capacity``: the first number of triples to try;
    the call is repeated with room for what the library reports until the table is whole."""
    tile_a, tile_b = as_label_tile(tile_a, "tile a"), as_label_tile(tile_b, "tile b")
    ndim = len(tile_a.shape)
    if len(tile_b.shape) != ndim:
        raise ValueError("the two tiles differ in rank")
    box_lo, box_n = [int(v) for v in box_lo], [int(v) for v in box_n]
    if len(box_lo) != ndim or len(box_n) != ndim:
        raise ValueError(f"the box needs {ndim} values per corner")
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint64))
    if min(box_n) < 1:
        return empty
    lib = _lib.init(device)
    va, keep_a = label_view(tile_a, None, None, device)
    vb, keep_b = label_view(tile_b, matrix, offset, device)
    capacity = PAIR_CAPACITY if capacity is None else int(capacity)
    if capacity < 1:
        raise ValueError("capacity must be >= 1")
    lo3, n3 = _lib.i64x3([0] * (3 - ndim) + box_lo), _lib.i64x3([1] * (3 - ndim) + box_n)
    while True:
        la, lb, n = np.empty(capacity, np.int32), np.empty(capacity, np.int32), np.empty(capacity, np.uint64)
        n_unique = C.c_int64()
        rc = lib.mvs_label_pair_overlaps(device, C.byref(va), C.byref(vb), ndim, lo3, n3, capacity, la.ctypes.data_as(C.POINTER(C.c_int32)),
                                         lb.ctypes.data_as(C.POINTER(C.c_int32)), n.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n_unique))
        if rc == _lib.MVS_LABEL_INCOMPLETE:
            bigger = max(int(n_unique.value), 2 * capacity)
            if bigger > _lib.MVS_LABEL_PAIR_MAX_CAPACITY and capacity == _lib.MVS_LABEL_PAIR_MAX_CAPACITY:
                raise _lib.MvsError(f"mvs_label_pair_overlaps: more than {capacity} distinct label pairs in one overlap", _lib.ERR_UNSUPPORTED)
            capacity = min(bigger, _lib.MVS_LABEL_PAIR_MAX_CAPACITY)
            continue
        _lib.check(rc, device, "mvs_label_pair_overlaps")
        break
    del keep_a, keep_b
    k = int(n_unique.value)
    order = np.lexsort((lb[:k], la[:k]))
    return la[:k][order], lb[:k][order], n[:k][order]


def fuse_label_tiles(tiles, matrices, offsets, luts, out_shape, index_origin=None, device=0, out_on_device=False):
    """The int32 label volume of shape ``out_shape`` (mvs_label_tiles_fuse): per voxel the label of the interior-most view in bounds,
    through that view's look-up table.  ``matrices[i]``, ``offsets[i]`` map an index of the frame to a pixel of view ``i``;
    ``index_origin``: the frame index of the output's first voxel (default zeros).  ``luts``: None, or per view None (the identity)
    or an int32 table with ``lut[label]`` the output id."""
    tiles = [as_label_tile(t, f"tile {i}") for i, t in enumerate(tiles)]
    if not tiles:
        raise ValueError("no tiles")
    ndim = len(out_shape)
    if ndim not in (2, 3) or any(len(t.shape) != ndim for t in tiles):
        raise ValueError("fuse_label_tiles needs 2-D or 3-D tiles and an output shape of the same rank")
    if luts is not None and len(luts) != len(tiles):
        raise ValueError("one look-up table (or None) per tile")
    origin = [0] * ndim if index_origin is None else [int(v) for v in index_origin]
    if len(origin) != ndim:
        raise ValueError(f"index_origin needs {ndim} values")
    lib = _lib.init(device)
    views = (_lib.mvs_view_t * len(tiles))()
    keep = []
    for i, (tile, matrix, offset) in enumerate(zip(tiles, matrices, offsets)):
        views[i], kept = label_view(tile, matrix, offset, device)
        keep.append(kept)
    lut_ptrs, lut_lens = None, None
    if luts is not None and any(t is not None for t in luts):
        # all tables in one device block, each on a 16-byte boundary
        hosts = [None if t is None else np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in luts]
        if any(t is not None and t.size < 1 for t in hosts):
            raise ValueError("a look-up table needs at least the entry of label 0")
        starts, total = [], 0
        for t in hosts:
            starts.append(total)
            total += 0 if t is None else (t.size + 3) // 4 * 4
        block = np.zeros(max(total, 1), dtype=np.int32)
        for t, s in zip(hosts, starts):
            if t is not None:
                block[s:s + t.size] = t
        dev_block = DeviceArray.empty(block.shape, np.int32, device)
        _lib.check(lib.mvs_memcpy_h2d(device, dev_block.ptr, block.ctypes.data, block.nbytes), device, "h2d")
        keep.append(dev_block)
        lut_ptrs = (C.c_void_p * len(tiles))(*[None if t is None else dev_block.ptr + 4 * s for t, s in zip(hosts, starts)])
        lut_lens = (C.c_int64 * len(tiles))(*[0 if t is None else t.size for t in hosts])
    out, ptr, mem = result_array(out_shape, np.int32, out_on_device, device)
    _lib.check(lib.mvs_label_tiles_fuse(device, views, len(tiles), ndim, lut_ptrs, lut_lens, _lib.i64x3(shape3(out_shape)),
                                        _lib.i64x3([0] * (3 - ndim) + origin), C.c_void_p(ptr), mem), device, "mvs_label_tiles_fuse")
    del keep
    return written(out)


def as_image_tile(data, who="tile"):
    """An image tile as mvs_label_components takes it: a 2-D / 3-D uint8 / uint16 / float32 array, in host memory (made
    C-contiguous) or a DeviceArray with contiguous rows (strided windows are fine).  Nothing is converted: another dtype raises
    TypeError."""
    if not is_device_array(data):
        data = np.asarray(data)
    if np.dtype(data.dtype) not in _lib.DTYPE_CODES:
        raise TypeError(f"{who}: image tiles are uint8, uint16 or float32, not {data.dtype}")
    if len(data.shape) not in (2, 3):
        raise ValueError(f"{who}: tiles are 2-D or 3-D")
    if is_device_array(data):
        if data.strides[-1] != 1 and data.shape[-1] > 1:
            raise TypeError(f"{who}: device tiles need contiguous rows (stride 1 along x)")
        return data
    return np.ascontiguousarray(data)


def label_components(tile, threshold, connectivity=1, min_voxels=1, device=0, out_on_device=False):
    """``(labels, n)``: the connected components of the voxels of ``tile`` with ``(float32)v > (float32)threshold``, numbered as
    ``scipy.ndimage.label`` numbers them under ``generate_binary_structure(ndim, connectivity)`` (mvs_label_components).  ``tile``: a
    uint8 / uint16 / float32 host array or DeviceArray; ``threshold=None`` requires uint8 and means 0 (a mask).  Components with
    fewer than ``min_voxels`` voxels become 0 and the others keep the ids ``1 .. n`` in order.  ``labels`` is int32 of the tile's
    shape: a resident DeviceArray when ``out_on_device`` or when the tile is resident, else a numpy array."""
    tile = as_image_tile(tile)
    ndim = len(tile.shape)
    if threshold is None:
        if np.dtype(tile.dtype) != np.uint8:
            raise TypeError(f"threshold=None labels a uint8 mask; a {tile.dtype} tile needs a threshold")
        threshold = 0.0
    threshold = float(np.float32(threshold))      # what the kernel compares with
    connectivity, min_voxels = int(connectivity), int(min_voxels)
    if not 1 <= connectivity <= ndim:
        raise ValueError(f"connectivity must be 1 .. {ndim}, not {connectivity}")
    if int(np.prod(tile.shape, dtype=np.int64)) < 1:
        raise ValueError("an empty tile")
    lib = _lib.init(device)
    view, keep = label_view(tile, None, None, device)
    view.dtype = _lib.DTYPE_CODES[np.dtype(tile.dtype)]
    out, ptr, mem = result_array(tile.shape, np.int32, out_on_device or is_device_array(tile), device)
    n = C.c_int64()
    _lib.check(lib.mvs_label_components(device, C.byref(view), ndim, threshold, connectivity, max(min(min_voxels, 2**63 - 1), 0), C.c_void_p(ptr), mem,
                                        C.byref(n)), device, "mvs_label_components")
    del keep
    return written(out), int(n.value)
