"""Thin array-level wrappers of the non-rigid refinement entry points of libmvs_hip.so (mvs_block_match, mvs_field_warp).  The cell
rule and the interpolation tables are those of ``_intensity_ops``."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._intensity_ops import apply_to_tile, axis_table
from ._metric_ops import box3, moments_in_groups, pair_call_views
from .transformation import shape3


def n_shifts(radius):
    """Shifts of a search window of ``radius`` per axis: ``prod (2 r + 1)``."""
    return int(np.prod([2 * int(r) + 1 for r in radius]))


def block_match(fixed, moving, fixed_affine, moving_affine, blocks, radius, halfspaces=None, device=0, batch=None):
    """Moments of the sample pairs ``(f(g), m(g + s))`` per block and integer shift (mvs_block_match): a ``(B, S, 6)`` float64
    array with the rows ``(n, mean_f, mean_m, M2_f, M2_m, C_fm)``, ``S = prod (2 r + 1)``, the shift index z slowest and x fastest,
    each axis from ``-r`` to ``r``.

    ``fixed`` / ``moving``: 2-D / 3-D tiles of one dtype, numpy arrays or ``DeviceArray`` windows; ``fixed_affine`` /
    ``moving_affine = (matrix, offset)`` map a grid index to a pixel of the tile.  ``blocks``: int64 array ``(B, >= 2, ndim)`` with
    the rows ``lo, n`` first (``nonrigid.plan_blocks``); ``radius``: per axis.  ``halfspaces`` as in ``_metric_ops.pair_moments``.
    Blocks go to the device in groups of ``batch`` (default and at most MVS_BLOCKMATCH_MAX_BLOCKS, and no more than keep a group's
    result within MVS_BLOCKMATCH_MAX_RESULT_BYTES); a block's rows do not depend on its group."""
    lib = _lib.init(device)
    blocks = np.asarray(blocks, dtype=np.int64)
    ndim = len(radius)
    if ndim not in (2, 3) or blocks.ndim != 3 or blocks.shape[1] < 2 or blocks.shape[2] != ndim:
        raise ValueError("block_match needs a 2-D or 3-D radius and blocks of shape (B, >= 2, ndim)")
    S = n_shifts(radius)
    limit = max(1, min(_lib.MVS_BLOCKMATCH_MAX_BLOCKS, _lib.MVS_BLOCKMATCH_MAX_RESULT_BYTES // (S * 8 * _lib.MVS_PAIR_MOMENTS_LEN)))
    batch = limit if batch is None else int(batch)
    if not 1 <= batch <= limit:
        raise ValueError(f"batch must be 1..{limit}")
    fview, mview, hs_ptr, n_hs, keep = pair_call_views(fixed, moving, fixed_affine, moving_affine, halfspaces, ndim, device)
    r3 = _lib.i32x3(radius, ndim, 0)

    def call(group):
        recs = (_lib.mvs_block_t * len(group))()
        for rec, row in zip(recs, box3(group[:, :2])):
            rec.lo[:], rec.n[:] = row
        res = np.zeros((len(group), S, _lib.MVS_PAIR_MOMENTS_LEN))
        _lib.check(lib.mvs_block_match(device, C.byref(fview), C.byref(mview), ndim, hs_ptr, n_hs, recs, len(group), r3, res.ctypes.data_as(C.POINTER(C.c_double))),
                   device, "mvs_block_match")
        return res

    return moments_in_groups(blocks, batch, call, per_row=(S,))      # (`keep` lives until here)


def warp_field(data, field, out=None, out_dtype=None, device=0):
    """``data(clamp(p + d(p), 0, n - 1))`` for one 2-D / 3-D tile (mvs_field_warp).  ``field``: float32 ``nodes + (ndim,)``, one
    displacement in pixels (z, y, x) per cell, interpolated multilinearly between the cell centres; the value is read with the
    library's linear sampler.  ``data``: numpy array or (possibly strided) ``DeviceArray``; the result is of the same kind, of
    ``out_dtype`` (the input's dtype, the default, or float32).  ``out``: where the result goes -- a contiguous array of the data's
    shape and ``out_dtype`` that does not overlap ``data`` (the kernel gathers)."""
    lib = _lib.init(device)
    field = np.ascontiguousarray(field, dtype=np.float32)
    ndim = field.ndim - 1
    if ndim not in (2, 3) or field.shape[-1] != ndim or len(data.shape) != ndim:
        raise ValueError("warp_field needs a 2-D or 3-D tile and a field of shape nodes + (ndim,)")
    if not np.all(np.isfinite(field)):
        raise ValueError("warp_field needs a finite field")
    nodes = field.shape[:-1]
    field3 = np.zeros(tuple(shape3(nodes)) + (3,), dtype=np.float32)
    field3[..., 3 - ndim:] = field.reshape(tuple(shape3(nodes)) + (ndim,))
    tables = np.concatenate([part.view(np.uint8) for n, g in zip(shape3(data.shape), shape3(nodes)) for part in axis_table(n, g)])
    return apply_to_tile("mvs_field_warp", data, out, out_dtype, device, lambda view, out_ptr, out_code, out_mem: lib.mvs_field_warp(
        device, view, ndim, _lib.i32x3(nodes, ndim, 1), field3.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(tables.ctypes.data), out_ptr, out_code, out_mem))
