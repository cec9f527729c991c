"""Thin array-level wrapper of the registration metrics entry point of libmvs_hip.so (mvs_pair_moments), the NCC its moments give,
and the call frame it shares with the other pair-moment wrappers (``_intensity_ops.cell_pair_moments``, ``_nonrigid_ops.block_match``)."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._operands import embed3, shape3, tile_view

_DP = C.POINTER(C.c_double)


def pair_call_views(fixed, moving, fixed_affine, moving_affine, halfspaces, ndim, device):
    """``(fview, mview, hs_ptr, n_hs, keep)``: the ``tile_view`` of both tiles, the halfspace rows ``(a.., b)`` embedded as
    ``(a_z, a_y, a_x, b)`` (2-D: ``a_z = 0``) behind a double pointer (None without halfspaces), their count, and what must stay
    alive until the last call has returned (its last item is the embedded array)."""
    fview, keep_f = tile_view(fixed, fixed_affine[0], fixed_affine[1], device)
    mview, keep_m = tile_view(moving, moving_affine[0], moving_affine[1], device)
    hs = np.zeros((0, ndim + 1)) if halfspaces is None else np.asarray(halfspaces, dtype=np.float64).reshape(-1, ndim + 1)
    if len(hs) > _lib.MVS_PAIR_MAX_HALFSPACES:
        raise ValueError(f"at most {_lib.MVS_PAIR_MAX_HALFSPACES} halfspaces")
    hs3 = np.zeros((len(hs), 4))
    hs3[:, 3 - ndim:] = hs
    return fview, mview, hs3.ctypes.data_as(_DP) if len(hs3) else None, len(hs3), (keep_f, keep_m, hs3)


def moments_in_groups(rows, batch, call, per_row=()):
    """``call(group) -> moments`` over groups of at most ``batch`` consecutive ``rows``: the zero-filled float64 array
    ``(N,) + per_row + (6,)`` of all of them, in input order."""
    out = np.zeros((len(rows),) + tuple(per_row) + (_lib.MVS_PAIR_MOMENTS_LEN,))
    for i0 in range(0, len(rows), batch):
        out[i0:i0 + batch] = call(rows[i0:i0 + batch])
    return out


def box3(rows, fill=(0, 1)):
    """Integer rows ``(..., R, ndim)`` of 2-D or 3-D calls on three axes, as nested lists: row ``r`` gets ``fill[r]`` along the z that
    a 2-D row lacks (boxes ``lo, n``: 0 and 1).  One call per group: conversions per record are what a large group spends its time in."""
    rows = np.asarray(rows)
    if rows.shape[-1] == 3:
        return rows.tolist()
    out = np.empty(rows.shape[:-1] + (3,), dtype=np.int64)
    out[..., 0], out[..., 1:] = fill, rows
    return out.tolist()


def pair_moments(fixed, moving, fixed_affine, cand_affines, grid_shape, halfspaces=None, device=0):
    """Moments of the sample pairs of two tiles over a grid (mvs_pair_moments): an ``(K, 6)`` float64 array with the rows
    ``(n, mean_f, mean_m, M2_f, M2_m, C_fm)``, one per candidate.

    ``fixed`` / ``moving``: 2-D / 3-D tiles of one dtype (uint8, uint16 or float32), numpy arrays or (possibly strided)
    ``DeviceArray`` windows, which are read in place.  ``fixed_affine = (matrix, offset)`` maps a grid index to a fixed pixel,
    ``cand_affines`` is a sequence of such pairs that map a grid index to a moving pixel.  ``halfspaces``: rows ``(a.., b)`` in grid
    index coordinates; a voxel counts only if ``a . index + b <= 0`` for every row (none: every voxel).  Candidates go to the
    device in groups of MVS_PAIR_MAX_CANDIDATES; a candidate's row does not depend on its group."""
    lib = _lib.init(device)
    grid_shape = tuple(int(s) for s in grid_shape)
    ndim = len(grid_shape)
    if ndim not in (2, 3):
        raise ValueError("pair_moments needs a 2-D or 3-D grid")
    fview, mview, hs_ptr, n_hs, keep = pair_call_views(fixed, moving, fixed_affine, (np.eye(ndim), np.zeros(ndim)), halfspaces, ndim, device)
    embedded = [embed3(np.asarray(m, dtype=np.float64), np.asarray(o, dtype=np.float64)) for m, o in cand_affines]

    def call(group):
        cm = np.ascontiguousarray([m.reshape(9) for m, _ in group], dtype=np.float64)
        co = np.ascontiguousarray([o for _, o in group], dtype=np.float64)
        res = np.zeros((len(group), _lib.MVS_PAIR_MOMENTS_LEN))
        _lib.check(lib.mvs_pair_moments(device, C.byref(fview), C.byref(mview), len(group), cm.ctypes.data_as(_DP), co.ctypes.data_as(_DP), ndim,
                                        _lib.i64x3(shape3(grid_shape)), hs_ptr, n_hs, res.ctypes.data_as(_DP)), device, "mvs_pair_moments")
        return res

    return moments_in_groups(embedded, _lib.MVS_PAIR_MAX_CANDIDATES, call)      # (`keep` lives until here)


def ncc_from_moments(m):
    """The normalised cross-correlation of one row of ``pair_moments`` by the rule of the reference (metrics.py:62-79): NaN with
    fewer than two sample pairs or when ``sqrt(M2_f * M2_m) < 1e-10`` (a constant image), else ``C_fm / sqrt(M2_f * M2_m)``."""
    n, _, _, m2f, m2m, cfm = (float(v) for v in m)
    if n < 2:
        return float("nan")
    denom = math.sqrt(m2f * m2m)
    if denom < 1e-10:
        return float("nan")
    return float(cfm / denom)
