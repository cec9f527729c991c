"""Thin array-level wrapper of the PSF extraction entry point of libmvs_hip.so (mvs_psf_extract) and the host geometry its
callers need: the window matrix and the separation rule."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._operands import tile_view

STATUS_USED, STATUS_OUTSIDE, STATUS_EMPTY = 0, 1, 2      # status_out of mvs_psf_extract


def window_matrix(spacing, linear, output_spacing):
    """``M = diag(1 / spacing) L^-1 diag(output_spacing)``: an offset in output-grid voxels -> an offset in view pixels, for a view
    with pixel ``spacing`` whose view -> world affine has the linear part ``L``.  A singular ``L`` raises ``ValueError``."""
    spacing = np.asarray(spacing, dtype=np.float64)
    out = np.asarray(output_spacing, dtype=np.float64)
    lin = np.asarray(linear, dtype=np.float64)
    ndim = len(spacing)
    if lin.shape != (ndim, ndim) or out.shape != (ndim,):
        raise ValueError(f"the linear part must be {ndim} x {ndim} and output_spacing have {ndim} entries")
    if not (np.all(np.isfinite(lin)) and np.all(np.isfinite(out)) and np.all(out > 0) and np.all(spacing > 0)):
        raise ValueError("affine and spacings must be finite, spacings positive")
    if np.linalg.matrix_rank(lin) < ndim:
        raise ValueError("the affine is singular: it has no inverse to map output-grid offsets into the view")
    return np.diag(1.0 / spacing) @ np.linalg.inv(lin) @ np.diag(out)


def too_close(centers, matrix, radius):
    """Boolean mask of the beads whose windows hold another bead's centre: for a pair (a, b), ``d = M^-1 (c_b - c_a)`` with
    ``|d_k| < 2 r_k + 1`` on every axis marks both.  The pairs come from a k-d tree on the scaled coordinates (no n x n array)."""
    from scipy.spatial import cKDTree

    centers = np.asarray(centers, dtype=np.float64)
    mask = np.zeros(len(centers), dtype=bool)
    if len(centers) < 2:
        return mask
    q = np.linalg.solve(np.asarray(matrix, dtype=np.float64), centers.T).T / (2.0 * np.asarray(radius, dtype=np.float64) + 1.0)
    pairs = cKDTree(q).query_pairs(1.0, p=np.inf, output_type="ndarray")
    if len(pairs):
        strict = np.all(np.abs(q[pairs[:, 0]] - q[pairs[:, 1]]) < 1.0, axis=1)      # (the tree's bound is <=)
        mask[pairs[strict].reshape(-1)] = True
    return mask


def psf_extract(data, centers, matrix, radius, refine_iterations=1, device=0):
    """mvs_psf_extract on one view.  ``data``: 2-D / 3-D uint8 / uint16 / float32, a numpy array or a ``DeviceArray`` (read in
    place); ``centers``: (n, ndim) pixel coordinates; ``matrix``: (ndim, ndim) window matrix; ``radius``: ndim integers in
    1 .. MVS_PSF_MAX_RADIUS.  Returns ``(psf, centers_out, status, stats)``: the float32 average window of shape ``2 radius + 1``
    (all zero when no bead is used), the (n, ndim) centres the beads were last sampled at, the (n,) int32 status codes and the
    (n, 3) float32 rows (background, energy sum, correlation with the average)."""
    lib = _lib.init(device)
    ndim = len(data.shape)
    centers = np.asarray(centers, dtype=np.float64)
    if ndim not in (2, 3) or centers.ndim != 2 or centers.shape[1] != ndim or len(centers) < 1:
        raise ValueError("psf_extract needs a 2-D or 3-D view and an (n >= 1, ndim) array of centres")
    radius = [int(r) for r in radius]
    if len(radius) != ndim or min(radius) < 1 or max(radius) > _lib.MVS_PSF_MAX_RADIUS:
        raise ValueError(f"one radius per axis in 1..{_lib.MVS_PSF_MAX_RADIUS}")
    n, k = len(centers), 3 - ndim
    view, keep = tile_view(data, np.eye(ndim), np.zeros(ndim), device)
    c3 = np.zeros((n, 3))
    c3[:, k:] = centers
    m3 = np.eye(3)
    m3[k:, k:] = np.asarray(matrix, dtype=np.float64)
    r3 = (C.c_int32 * 3)(*([0] * k + radius))
    out_c = np.zeros((n, 3))
    status = np.zeros(n, dtype=np.int32)
    stats = np.zeros((n, 3), dtype=np.float32)
    psf = np.zeros(tuple(2 * r + 1 for r in radius), dtype=np.float32)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    m3 = np.ascontiguousarray(m3.reshape(9))
    rc = lib.mvs_psf_extract(device, C.byref(view), ndim, c3.ctypes.data_as(dp), n, m3.ctypes.data_as(dp), r3, int(refine_iterations),
                             out_c.ctypes.data_as(dp), status.ctypes.data_as(C.POINTER(C.c_int32)), stats.ctypes.data_as(fp),
                             psf.ctypes.data_as(fp))
    _lib.check(rc, device, "mvs_psf_extract")
    del keep
    return psf, out_c[:, k:], status, stats
