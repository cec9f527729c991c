"""Thin array-level wrapper of the registration metrics entry point of libmvs_hip.so (mvs_pair_moments) and the NCC its moments
give."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .transformation import embed3, shape3, tile_view


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
    fview, keep_f = tile_view(fixed, fixed_affine[0], fixed_affine[1], device)
    mview, keep_m = tile_view(moving, np.eye(ndim), np.zeros(ndim), device)
    hs = np.zeros((0, ndim + 1)) if halfspaces is None else np.asarray(halfspaces, dtype=np.float64).reshape(-1, ndim + 1)
    if len(hs) > _lib.MVS_PAIR_MAX_HALFSPACES:
        raise ValueError(f"at most {_lib.MVS_PAIR_MAX_HALFSPACES} halfspaces")
    hs3 = np.zeros((len(hs), 4))
    hs3[:, 3 - ndim:] = hs                       # 2-D: a_z = 0
    embedded = [embed3(np.asarray(m, dtype=np.float64), np.asarray(o, dtype=np.float64)) for m, o in cand_affines]
    out = np.zeros((len(embedded), _lib.MVS_PAIR_MOMENTS_LEN))
    dp = C.POINTER(C.c_double)
    for k0 in range(0, len(embedded), _lib.MVS_PAIR_MAX_CANDIDATES):
        group = embedded[k0:k0 + _lib.MVS_PAIR_MAX_CANDIDATES]
        cm = np.ascontiguousarray([m.reshape(9) for m, _ in group], dtype=np.float64)
        co = np.ascontiguousarray([o for _, o in group], dtype=np.float64)
        res = np.zeros((len(group), _lib.MVS_PAIR_MOMENTS_LEN))
        rc = lib.mvs_pair_moments(device, C.byref(fview), C.byref(mview), len(group), cm.ctypes.data_as(dp), co.ctypes.data_as(dp), ndim,
                                  _lib.i64x3(shape3(grid_shape)), hs3.ctypes.data_as(dp) if len(hs3) else None, len(hs3),
                                  res.ctypes.data_as(dp))
        _lib.check(rc, device, "mvs_pair_moments")
        out[k0:k0 + len(group)] = res
    del keep_f, keep_m
    return out


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
