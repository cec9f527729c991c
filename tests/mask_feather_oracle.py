"""The scipy restatement of ``masks.feather`` (mvs_mask_feather): numpy and scipy only.

``W = rint(252 * (1 - cos(pi * min(t, 1))) / 2)`` with ``t`` the Euclidean distance to the nearest zero voxel of the mask in units of
the feather width per axis -- ``scipy.ndimage.distance_transform_edt(mask != 0, sampling=1 / w)`` -- in float64.  Voxels outside
the array are not zero voxels; a mask without a zero is all 252 (scipy's transform has no meaning without a background and is not
called)."""
import numpy as np
from scipy import ndimage

FULL_WEIGHT = 252


def widths_of(width, ndim):
    """One width per axis; the one number 0 (no feather) is width 1."""
    if np.ndim(width) == 0:
        return [max(int(width), 1)] * ndim
    assert len(width) == ndim
    return [int(w) for w in width]


def capped_distance(mask, width):
    """``min(t, 1)`` in float64."""
    mask = np.asarray(mask) != 0
    if mask.all():
        return np.ones(mask.shape, dtype=np.float64)
    w = widths_of(width, mask.ndim)
    return np.minimum(ndimage.distance_transform_edt(mask, sampling=[1.0 / k for k in w]), 1.0)


def ramp(t):
    """The weight before rounding, float64."""
    return FULL_WEIGHT * 0.5 * (1.0 - np.cos(np.pi * np.minimum(np.asarray(t, dtype=np.float64), 1.0)))


def feather_float(mask, width):
    return ramp(capped_distance(mask, width))


def feather(mask, width):
    return np.rint(feather_float(mask, width)).astype(np.uint8)


def half_integer_distance(values):
    """How far the values before rounding stay from a half-integer (where a last-ulp difference of two cosines could flip a byte)."""
    v = np.asarray(values, dtype=np.float64)
    return float(np.abs(v - np.floor(v) - 0.5).min()) if v.size else 0.5


def brute_force_distance(mask, width):
    """``min(t, 1)`` from the definition: every voxel against every zero voxel, float64.  For tiny masks."""
    mask = np.asarray(mask) != 0
    w = np.asarray(widths_of(width, mask.ndim), dtype=np.float64)
    zeros = np.argwhere(~mask).astype(np.float64)
    out = np.ones(mask.shape, dtype=np.float64)
    if not len(zeros):
        return out
    for p in np.ndindex(*mask.shape):
        out[p] = min(np.sqrt((((np.asarray(p, dtype=np.float64) - zeros) / w) ** 2).sum(1).min()), 1.0)
    return out
