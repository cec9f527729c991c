"""What the fusion functions of the stack kind share (``mv_deconv``, ``multiband``): the input half of the public function, which
turns ``transformed_views`` / ``blending_weights`` into device float32 stacks (V, *S), and the frame of the call into the library
that fuses such a stack (mvs_mv_deconv, mvs_multiband_fuse: csrc/mvs_stack_frame.h is the same frame on the C++ side)."""

from __future__ import annotations

import numpy as np

from . import _lib
from ._operands import dense_operand, result_array, written
from .device import DeviceArray, is_device_array


def stack_dims(name, transformed_views, blending_weights):
    """``(n_views, ndim)`` of a stack (n_views, [z,] y, x) and its weights, or the ``ValueError`` of ``name``.  Touches no device."""
    ndim = len(transformed_views.shape) - 1
    if ndim not in (2, 3):
        raise ValueError(f"{name} fuses 2D or 3D views: transformed_views is (n_views, [z,] y, x)")
    if tuple(blending_weights.shape) != tuple(transformed_views.shape):
        raise ValueError("blending_weights must have the shape of transformed_views")
    return int(transformed_views.shape[0]), ndim


def stack_inputs(name, transformed_views, blending_weights, device):
    """The inputs of the fusion function ``name`` as ``(views, weights, ndim, out_dtype, out_on_device, cast_dtype)``.

    ``DeviceArray`` views (contiguous float32, else ``TypeError``; host weights are uploaded) stay where they are, and so does the
    float32 result: ``cast_dtype`` is None.  Host views are uploaded as float32; the result comes back to the host in their dtype
    where the library writes it (uint8, uint16, float32), else in float32, and is cast to ``cast_dtype``, the views' dtype."""
    _, ndim = stack_dims(name, transformed_views, blending_weights)
    if is_device_array(transformed_views):
        if not is_device_array(blending_weights):
            blending_weights = DeviceArray.from_host(np.ascontiguousarray(blending_weights, dtype=np.float32), device)
        views, weights = (dense_operand(a, (np.float32,), device, f"device inputs of {name}")[2] for a in (transformed_views, blending_weights))
        return views, weights, ndim, np.dtype(np.float32), True, None
    host = np.asarray(transformed_views)
    views = DeviceArray.from_host(np.ascontiguousarray(host, dtype=np.float32), device)
    weights = DeviceArray.from_host(np.ascontiguousarray(blending_weights, dtype=np.float32), device)
    out_dtype = host.dtype if host.dtype in _lib.DTYPE_CODES else np.dtype(np.float32)
    return views, weights, ndim, out_dtype, False, host.dtype


def run_stack_call(name, views, ndim, trim, out_dtype, out_on_device, device, out, call):
    """One call of the entry point ``name`` on a device stack ``views`` (V, *S): the result, trimmed by ``trim`` (per spatial axis)
    and cast to ``out_dtype``, as a DeviceArray (``out_on_device``; ``out``: a contiguous DeviceArray of the result shape and dtype to
    write into) or a numpy array.  ``call(shape3, t3, out_dtype_code, out_ptr, out_mem)`` fills the entry's own options around the
    shape and trim as (z, y, x), calls the library and returns its code."""
    shape3 = (1,) * (3 - ndim) + tuple(views.shape[1:])
    t3 = [0] * (3 - ndim) + [int(t) for t in trim]
    res_shape = tuple(s - 2 * t for s, t in zip(views.shape[1:], trim))
    out, optr, omem = result_array(res_shape, out_dtype, out_on_device, device, out if out_on_device else None)
    _lib.check(call(shape3, t3, _lib.DTYPE_CODES[np.dtype(out_dtype)], optr, omem), device, name)
    return written(out)
