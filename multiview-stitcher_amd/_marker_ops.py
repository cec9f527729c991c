"""Thin array-level wrappers of the marker-registration entry points of libmvs_hip.so (mvs_knn, mvs_marker_descriptors,
mvs_marker_score).  Point and descriptor sets are (n, dim) float64, numpy arrays or contiguous DeviceArrays."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._operands import dense_operand, result_array, written
from .device import DeviceArray, is_device_array


def to_device(rows, device=0):
    """An (n, dim) float64 set as a resident DeviceArray (descriptors and points that several queries read)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    out = DeviceArray.empty(rows.shape, np.float64, device)
    out._buf.upload(rows)
    return out


def _point_set(a, device, what):
    """(pointer, mem code, keep-alive, shape) of an (n, dim) float64 set."""
    ptr, mem, a = dense_operand(a, (np.float64,), device, what, host_dtype=np.float64)
    if len(a.shape) != 2:
        raise (TypeError if is_device_array(a) else ValueError)(f"{what}: expected an (n, dim) array")
    return ptr, mem, a, a.shape


def knn(ref, query, k, device=0):
    """The ``k`` nearest rows of ``ref`` for every row of ``query`` (mvs_knn): ``(indices int32, distances float64)``, both
    (n_query, k), ascending by distance, equal distances by ascending index; with k > n_ref the tail is -1 / +inf.  ``dim``
    above 15 or ``k`` above 16 raise NotImplementedError: there is no CPU fallback."""
    rp, rmem, rkeep, rshape = _point_set(ref, device, "knn")
    same = query is ref
    qp, qmem, qkeep, qshape = (rp, rmem, rkeep, rshape) if same else _point_set(query, device, "knn")
    if rshape[1] != qshape[1]:
        raise ValueError("knn: reference and query rows differ in length")
    dim, k = int(rshape[1]), int(k)
    if dim > _lib.MVS_KNN_MAX_DIM:
        raise NotImplementedError(f"knn: dim = {dim} exceeds the kernel's limit of {_lib.MVS_KNN_MAX_DIM}")
    if k > _lib.MVS_KNN_MAX_K:
        raise NotImplementedError(f"knn: k = {k} exceeds the kernel's limit of {_lib.MVS_KNN_MAX_K}")
    if k < 1 or dim < 1 or rshape[0] < 1 or qshape[0] < 1:
        raise ValueError("knn: k, dim and both row counts must be positive")
    lib = _lib.init(device)
    idx = np.empty((qshape[0], k), dtype=np.int32)
    dist = np.empty((qshape[0], k), dtype=np.float64)
    rc = lib.mvs_knn(device, C.c_void_p(rp), rmem, rshape[0], C.c_void_p(qp), qmem, qshape[0], dim, k,
                     idx.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(C.POINTER(C.c_double)))
    _lib.check(rc, device, "mvs_knn")
    return idx, dist


def check_descriptor_params(num_neighbors, redundancy):
    """The kernels' limits on the descriptor parameters, as NotImplementedError naming the parameter."""
    if num_neighbors > _lib.MVS_MARKER_MAX_NEIGHBORS:
        raise NotImplementedError(f"num_neighbors = {num_neighbors} exceeds the kernel's limit of {_lib.MVS_MARKER_MAX_NEIGHBORS}")
    if num_neighbors + redundancy > _lib.MVS_KNN_MAX_K - 2:
        raise NotImplementedError(f"num_neighbors + redundancy = {num_neighbors + redundancy} needs k > {_lib.MVS_KNN_MAX_K} in the "
                                  f"neighbourhood query: redundancy is limited to {_lib.MVS_KNN_MAX_K - 2 - num_neighbors} here")
    if math.comb(num_neighbors + redundancy, num_neighbors) + 1 > _lib.MVS_KNN_MAX_K:
        raise NotImplementedError(f"redundancy = {redundancy} gives {math.comb(num_neighbors + redundancy, num_neighbors)} descriptors per "
                                  f"point: matching would need k > {_lib.MVS_KNN_MAX_K}")


def descriptors(points, neighbors, num_neighbors, redundancy, device=0, out_on_device=False):
    """The sorted pairwise-distance vectors of every point with every ``num_neighbors``-subset of its
    ``num_neighbors + redundancy`` neighbours (mvs_marker_descriptors): (n * C, L) float64, row p * C + s for point p and the
    s-th subset in itertools.combinations order.  ``neighbors``: (n, required) indices of each point's nearest other points."""
    num_neighbors, redundancy = int(num_neighbors), int(redundancy)
    check_descriptor_params(num_neighbors, redundancy)
    pp, pmem, pkeep, pshape = _point_set(points, device, "descriptors")
    required = num_neighbors + redundancy
    neighbors = np.ascontiguousarray(neighbors, dtype=np.int32)
    if neighbors.shape != (pshape[0], required):
        raise ValueError("descriptors: neighbors must be (n_points, num_neighbors + redundancy)")
    lib = _lib.init(device)
    rows = pshape[0] * math.comb(required, num_neighbors)
    length = math.comb(num_neighbors + 1, 2)
    out, optr, omem = result_array((rows, length), np.float64, out_on_device, device)
    rc = lib.mvs_marker_descriptors(device, C.c_void_p(pp), pmem, pshape[0], int(pshape[1]), neighbors.ctypes.data_as(C.POINTER(C.c_int32)),
                                    num_neighbors, redundancy, C.c_void_p(optr), omem)
    _lib.check(rc, device, "mvs_marker_descriptors")
    return written(out)


def score(affines, fixed, moving, max_error, device=0):
    """Per fixed -> moving affine of ``affines`` (H, ndim + 1, ndim + 1): the number of rows with
    ``||A f + t - m|| <= max_error`` (int32) and the sum of those residuals (float64) (mvs_marker_score)."""
    affines = np.ascontiguousarray(affines, dtype=np.float64)
    fixed = np.ascontiguousarray(fixed, dtype=np.float64)
    moving = np.ascontiguousarray(moving, dtype=np.float64)
    ndim = fixed.shape[1]
    if affines.ndim != 3 or affines.shape[1:] != (ndim + 1, ndim + 1) or moving.shape != fixed.shape:
        raise ValueError("score: affines must be (H, ndim + 1, ndim + 1), fixed and moving (C, ndim)")
    lib = _lib.init(device)
    counts = np.empty(len(affines), dtype=np.int32)
    sums = np.empty(len(affines), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    rc = lib.mvs_marker_score(device, affines.ctypes.data_as(dp), len(affines), fixed.ctypes.data_as(dp), moving.ctypes.data_as(dp),
                              len(fixed), ndim, float(max_error), counts.ctypes.data_as(C.POINTER(C.c_int32)), sums.ctypes.data_as(dp))
    _lib.check(rc, device, "mvs_marker_score")
    return counts, sums
