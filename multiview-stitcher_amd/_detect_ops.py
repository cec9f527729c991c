"""Thin array-level wrappers of the detection entry points of libmvs_hip.so (mvs_log_response, mvs_local_maxima) and the
host-side filter taps they take."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, is_device_array
from ._operands import dense_operand, shape3

# device bytes per voxel of a whole-field detection: the response and up to three work volumes of mvs_log_response (16), or the
# response, two running maxima and a smoothed sample volume of mvs_local_maxima (16)
WORK_BYTES_PER_VOXEL = 16


def gaussian_taps(sigma, order):
    """(radius, taps) of scipy.ndimage's Gaussian line filter for ``order`` 0 or 2 (truncate = 4): radius = int(4 sigma + 0.5),
    taps = phi / sum(phi) times the polynomial of the derivative (order 2: x^2 / sigma^4 - 1 / sigma^2), float64."""
    if order not in (0, 2):
        raise ValueError("order must be 0 or 2")
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    phi = phi / phi.sum()
    if order == 0:
        return radius, phi
    q = -1.0 / sigma2 + (x ** 2) * (1.0 / sigma2 * (1.0 / sigma2))
    return radius, q * phi


def fits_device(n_voxels, itemsize, on_host, device=0):
    """True when the work areas of a detection over ``n_voxels`` at once (plus the image, when it still has to be uploaded) fit
    into four fifths of the device memory that is free now (mvs_mem_info)."""
    free, _ = _lib.mem_info(device)
    need = int(n_voxels) * (WORK_BYTES_PER_VOXEL + (int(itemsize) if on_host else 0))
    return need <= 0.8 * free


def _filter(image, sigmas, with_second_order, scale, max_range, device):
    lib = _lib.init(device)
    shape = tuple(int(s) for s in image.shape)
    ndim = len(shape)
    if ndim not in (2, 3) or len(sigmas) != ndim:
        raise ValueError("detection needs a 2-D or 3-D image and one sigma per axis")
    dtype = np.dtype(image.dtype)
    if dtype not in _lib.DTYPE_CODES:
        raise TypeError(f"unsupported dtype {dtype} (uint8/uint16/float32)")
    tables = [gaussian_taps(s, 0) for s in sigmas]
    radius = [0] * (3 - ndim) + [r for r, _ in tables]
    if max(radius) > _lib.MVS_LOG_MAX_RADIUS:
        raise ValueError(f"filter radius {max(radius)} (sigma {max(sigmas):.3g} px) exceeds the kernel's limit of {_lib.MVS_LOG_MAX_RADIUS}")
    dp = C.POINTER(C.c_double)
    taps0 = np.ascontiguousarray(np.concatenate([t for _, t in tables]))
    taps2 = np.ascontiguousarray(np.concatenate([gaussian_taps(s, 2)[1] for s in sigmas])) if with_second_order else None
    ptr, mem, keep = dense_operand(image, _lib.DTYPE_CODES, device, "detection kernels")
    out = DeviceArray.empty(shape, np.float32, device)
    mx = C.c_float()
    rng = None if max_range is None else (C.c_int64 * 2)(int(max_range[0]), int(max_range[1]))
    rc = lib.mvs_log_response(device, ptr, _lib.DTYPE_CODES[dtype], mem, ndim, _lib.i64x3(shape3(shape)), (C.c_int32 * 3)(*radius),
                              taps0.ctypes.data_as(dp), None if taps2 is None else taps2.ctypes.data_as(dp), float(scale), rng,
                              C.c_void_p(out.ptr), C.byref(mx))
    _lib.check(rc, device, "mvs_log_response")
    out.mark_written()
    return out, np.float32(mx.value)


def log_response(image, sigmas, scale, max_range=None, device=0):
    """``-scipy.ndimage.gaussian_laplace(image.astype(float32), sigmas, mode="reflect") * scale`` on the GPU (mvs_log_response).
    ``image``: 2-D / 3-D uint8 / uint16 / float32, numpy or contiguous DeviceArray.  Returns (float32 DeviceArray, its maximum
    as numpy.float32); ``max_range = (lo, hi)`` restricts the maximum to those slices of the first axis."""
    return _filter(image, sigmas, True, scale, max_range, device)


def gaussian_smooth(image, sigmas, device=0):
    """``scipy.ndimage.gaussian_filter(image.astype(float32), sigmas)`` on the GPU: the order-0 passes of mvs_log_response."""
    return _filter(image, sigmas, False, 1.0, None, device)[0]


def local_maxima(response, window, threshold, sample=None, sample_window=None, bound=None, device=0, capacity=None):
    """The voxels of ``response`` (float32 DeviceArray) that equal the maximum over the odd box ``window``, exceed ``threshold``
    (compared in float32) and 0, and -- with ``sample`` -- whose minimum of ``sample`` (DeviceArray of the same shape) over the box
    ``sample_window`` lies below ``bound`` (mvs_local_maxima).  Returns an (n, ndim) int64 array in raster order.  The device
    list holds ``capacity`` entries; when there are more detections the call is repeated with a list that holds them all."""
    lib = _lib.init(device)
    if not is_device_array(response):
        raise TypeError("local_maxima needs a contiguous float32 DeviceArray")
    rptr, _, response = dense_operand(response, (np.float32,), device, "the response of local_maxima")
    shape = tuple(int(s) for s in response.shape)
    ndim = len(shape)
    pad = [1] * (3 - ndim)
    win = (C.c_int32 * 3)(*(pad + [int(w) for w in window]))
    sptr, sdtype, swin, bnd = None, _lib.MVS_F32, None, 0.0
    if sample is not None:
        if not is_device_array(sample) or tuple(sample.shape) != shape:
            raise TypeError("the sample volume must be a contiguous DeviceArray of the response's shape (uint8/uint16/float32)")
        ptr, _, sample = dense_operand(sample, _lib.DTYPE_CODES, device, "the sample volume of local_maxima")
        sptr, sdtype = C.c_void_p(ptr), _lib.DTYPE_CODES[sample.dtype]
        swin = (C.c_int32 * 3)(*(pad + [int(w) for w in sample_window]))
        bnd = float(bound)
    cap = 4096 if capacity is None else int(capacity)
    while True:
        buf = np.empty((max(cap, 1), 3), dtype=np.int32)
        count = C.c_int64()
        rc = lib.mvs_local_maxima(device, C.c_void_p(rptr), ndim, _lib.i64x3(shape3(shape)), win, float(np.float32(threshold)), sptr,
                                  sdtype, swin, bnd, buf.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(count))
        _lib.check(rc, device, "mvs_local_maxima")
        if count.value <= cap:
            break
        cap = int(count.value)
    pts = buf[:count.value, 3 - ndim:].astype(np.int64)
    order = np.lexsort(pts.T[::-1])
    return pts[order]
