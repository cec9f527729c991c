"""The operand step of the ctypes wrappers: how a numpy array or a ``DeviceArray`` becomes what a C entry point takes -- a
pointer, an ``MVS_MEM_*`` code and an object to keep alive -- and how a result array is made, handed over and marked as written.

One rule for every array argument: a ``DeviceArray`` is brought to the call's device (``on_device``: a peer copy when it lives on
another GPU) and the call's stream waits for an upload still in flight (``wait_ready``); two arrays of one call live on the same
side; a result goes through ``result_array`` and ``written``.  For a resident array with no pending upload on its own device
neither step makes a library call.

- ``dense_operand`` / ``operand_pair``: flat, contiguous arrays;
- ``view_data`` / ``fill_view_geometry`` / ``tile_view``: (possibly strided) 2-D / 3-D views as ``mvs_view_t``;
- ``result_array`` / ``written``: the result frame.
"""

from __future__ import annotations

import numpy as np

from . import _lib
from .device import DeviceArray, is_device_array


def shape3(shape):
    shape = [int(s) for s in shape]
    return [1] * (3 - len(shape)) + shape


def embed3(matrix, offset):
    """Embed an ndim-D pixel affine into the 3D (z,y,x) form the C ABI takes (2D: z -> z)."""
    ndim = len(offset)
    m3 = np.eye(3)
    o3 = np.zeros(3)
    k = 3 - ndim
    m3[k:, k:] = matrix
    o3[k:] = offset
    return m3, o3


def dense_operand(a, dtypes, device, what, host_dtype=None, error=TypeError):
    """``(pointer, MVS_MEM_* code, array to keep alive until the call is over)`` of a flat, contiguous input array.  A DeviceArray
    must be contiguous and of one of ``dtypes`` (else ``error`` naming ``what``); it is brought to ``device`` and the stream of
    that context waits for its upload.  A host array is made C-contiguous and cast to ``host_dtype`` if one is given."""
    if is_device_array(a):
        if not a.is_contiguous() or a.dtype not in dtypes:
            raise error(f"{what}: a DeviceArray must be contiguous and of dtype {' / '.join(np.dtype(d).name for d in dtypes)}")
        a = a.on_device(device)      # resident on another GPU: peer copy, cached per (allocation, device)
        a.wait_ready(device)         # still on its way (device.to_device_async)
        return a.ptr, _lib.MVS_MEM_DEVICE, a
    a = np.ascontiguousarray(a, dtype=host_dtype)
    return a.ctypes.data, _lib.MVS_MEM_HOST, a


def operand_pair(a, b, dtypes, device, what, host_dtype=None, names="images"):
    """``dense_operand`` of the two arrays of one call, which share one mem code: ``(pointer a, pointer b, mem, (keep a, keep b))``.
    Either may be None (an optional mask): its pointer is None and the other decides the side; two Nones count as host."""
    given = [x for x in (a, b) if x is not None]
    if len({is_device_array(x) for x in given}) > 1:
        raise TypeError(f"{what}: both {names} must live on the same side (host or device)")
    (pa, mem_a, ka), (pb, mem_b, kb) = ((None, None, None) if x is None else dense_operand(x, dtypes, device, what, host_dtype) for x in (a, b))
    return pa, pb, next((m for m in (mem_a, mem_b) if m is not None), _lib.MVS_MEM_HOST), (ka, kb)


def result_array(shape, dtype, on_device, device, out=None, what="out"):
    """``(out, pointer, MVS_MEM_* code)`` of a call's result: a new DeviceArray (``on_device``) or numpy array of ``shape`` and
    ``dtype``, or the caller's ``out``, which must be a contiguous array of that kind, shape and dtype (else ``ValueError``).  The
    stream of ``device`` waits for an upload into ``out`` that is still in flight.  Call ``written(out)`` after the entry point."""
    shape, dtype = tuple(int(s) for s in shape), np.dtype(dtype)
    if out is None:
        out = DeviceArray.empty(shape, dtype, device) if on_device else np.empty(shape, dtype=dtype)
    elif not (is_device_array(out) if on_device else isinstance(out, np.ndarray)) or tuple(out.shape) != shape or out.dtype != dtype \
            or not (out.is_contiguous() if on_device else out.flags.c_contiguous):
        raise ValueError(f"{what} must be a contiguous {'DeviceArray' if on_device else 'numpy array'} of the result shape and dtype")
    if on_device:
        out.wait_ready(device)
        return out, out.ptr, _lib.MVS_MEM_DEVICE
    return out, out.ctypes.data, _lib.MVS_MEM_HOST


def written(out):
    """After a call has written into ``out`` (``result_array``): a DeviceArray's allocation is told so (peer copies on other GPUs go
    stale); nothing for a numpy array.  Returns ``out``."""
    if is_device_array(out):
        out.mark_written()
    return out


def view_data(data, device, dtype=None, wait=True, allow=_lib.DTYPE_CODES):
    """Where the C entries find a view's voxels: ``(pointer, 3D shape, 3D element strides, MVS_MEM_* code, array to keep
    alive until the call is over)``.  A DeviceArray is used in place, first brought to ``device`` and this lane's stream made to
    wait for an upload still in flight; a host array is made C-contiguous, cast to ``dtype`` if one is given and to float32 if its
    own is none of ``allow`` (the kernels' dtypes; the label entries add int32).  2D data is a single z plane.

    ``wait=False`` skips the peer copy and the wait.  ``_reg_ops.bin_mean`` is the only caller that passes it: the lane that bins
    is made to wait by ``registration._bin_sim`` before it calls (the batched pre-binning of ``registration.py`` brings the tiles
    to its lane and waits there in the same way)."""
    if is_device_array(data):
        if dtype is not None and data.dtype != dtype:
            raise TypeError("all views of a chunk must share one dtype")
        if wait:
            data = data.on_device(device)     # a tile resident on another GPU: peer copy, cached per (tile, device)
            data.wait_ready(device)           # a tile still on its way (device.to_device_async)
        if data.dtype not in allow:
            raise TypeError(f"unsupported dtype {data.dtype}")
        ptr, st, mem = data.ptr, [int(v) for v in data.strides], _lib.MVS_MEM_DEVICE
    else:
        data = np.ascontiguousarray(data, dtype=dtype)
        if data.dtype not in allow:
            data = data.astype(np.float32)
        st = [int(np.prod(data.shape[k + 1:])) for k in range(data.ndim)]   # C order; numpy's strides of size-1 axes are arbitrary
        ptr, mem = data.ctypes.data, _lib.MVS_MEM_HOST
    s3 = shape3(data.shape)
    if len(st) == 2:
        st = [st[0] * s3[1], st[0], st[1]]
    return ptr, s3, st, mem, data


def fill_view_geometry(view, data_ptr, dtype_code, mem, shape, strides_elems, matrix, offset):
    """Fill the data/geometry half of an ``mvs_view_t``."""
    m3, o3 = embed3(matrix, offset)
    s3 = shape3(shape)
    st3 = [int(s) for s in strides_elems]
    if len(st3) == 2:  # 2D slab: a single z plane
        st3 = [st3[0] * s3[1], st3[0], st3[1]]
    view.data = data_ptr
    view.dtype = dtype_code
    view.mem = mem
    view.shape[:] = s3
    view.stride[:] = st3
    view.offset[:] = o3.tolist()
    view.matrix[:] = m3.reshape(-1).tolist()


def tile_view(data, matrix, offset, device):
    """``(mvs_view_t, array to keep alive)`` of one whole tile for the entry points that take tiles (metrics, PSF extraction,
    intensity, shading, resampling): ``view_data`` and ``fill_view_geometry`` with the tile's own dtype."""
    view = _lib.mvs_view_t()
    ptr, s3, st3, mem, keep = view_data(data, device)
    fill_view_geometry(view, ptr, _lib.DTYPE_CODES[np.dtype(keep.dtype)], mem, s3, st3, matrix, offset)
    return view, keep
