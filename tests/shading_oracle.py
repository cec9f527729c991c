"""numpy / scipy restatement of the shading correction (include/mvs_hip.h: mvs_stack_quantiles, mvs_plane_apply; intensity.py:
shading_from_planes, shading_coefficients): sort-based order statistics of a stack, the arithmetic of the shading model with a
dense least squares fit, and the float32 apply.  Written from the contract, not from the kernels: no radix digits, no strips."""
import numpy as np
from numpy.polynomial import legendre
from scipy import ndimage


def stack_of(tiles):
    """All planes of the tiles as one (n, H, W) array."""
    return np.concatenate([np.asarray(t).reshape((-1,) + tuple(t.shape[-2:])) for t in tiles], axis=0)


def stack_quantiles(tiles, q):
    """(planes float32 (n_q, H, W), counts int32 (H, W)): per pixel the sample of ascending rank floor((n - 1) * q) among the n
    values of the stack that are not NaN (np.sort puts NaNs last), -0 counted as +0; NaN where n == 0."""
    stack = stack_of(tiles)
    if stack.dtype.kind == "f":
        stack = stack + np.float32(0.0)                       # -0 + 0 = +0; everything else keeps its bits
        counts = (~np.isnan(stack)).sum(axis=0)
    else:
        counts = np.full(stack.shape[1:], stack.shape[0])
    ordered = np.sort(stack, axis=0)
    planes = []
    for qj in np.atleast_1d(q):
        rank = np.floor(np.maximum(counts - 1, 0).astype(np.float64) * float(qj)).astype(np.int64)
        plane = np.take_along_axis(ordered, rank[None], axis=0)[0].astype(np.float32)
        planes.append(np.where(counts > 0, plane, np.float32(np.nan)))
    return np.stack(planes).astype(np.float32), counts.astype(np.int32)


def unit(n):
    return np.zeros(1) if n == 1 else -1.0 + 2.0 * np.arange(n) / (n - 1)


def smooth(plane, valid, degree=None, sigma=None):
    """The three smoothings of shading_from_planes, the polynomial one by a dense least squares on the design matrix."""
    h, w = plane.shape
    if degree is not None:
        yy, xx = np.meshgrid(unit(h), unit(w), indexing="ij")
        cols = []
        for i in range(degree + 1):
            for j in range(degree + 1 - i):
                cols.append(legendre.legval(yy, np.eye(degree + 1)[i]) * legendre.legval(xx, np.eye(degree + 1)[j]))
        design = np.stack([c.ravel() for c in cols], axis=1)
        coef = np.linalg.lstsq(design[valid.ravel()], plane.ravel()[valid.ravel()], rcond=None)[0]
        return (design @ coef).reshape(h, w)
    if sigma is not None:
        num = ndimage.gaussian_filter(np.where(valid, plane, 0.0), sigma, mode="nearest")
        den = ndimage.gaussian_filter(valid.astype(np.float64), sigma, mode="nearest")
        ok = den > 1e-12
        res = np.where(ok, num / np.where(ok, den, 1.0), 0.0)
        return np.where(ok, res, res[ok].mean())
    return np.where(valid, plane, plane[valid].mean())


def shading_from_planes(planes, counts, darkfield=None, degree=4, sigma=None, min_samples=8, min_flat=0.1):
    planes = np.asarray(planes, dtype=np.float64)
    enough = np.asarray(counts) >= min_samples
    if isinstance(darkfield, str):
        dark = smooth(planes[0], enough & np.isfinite(planes[0]), degree, sigma)
    elif darkfield is None:
        dark = np.zeros(planes.shape[1:])
    else:
        dark = np.broadcast_to(np.asarray(darkfield, dtype=np.float64), planes.shape[1:]).copy()
    with np.errstate(invalid="ignore"):
        raw = planes[-1] - dark
    valid = enough & np.isfinite(raw)
    flat = smooth(np.where(valid, raw, 0.0), valid, degree, sigma)
    flat = flat / flat.mean()
    flat = np.maximum(flat, min_flat)
    return {"flatfield": flat.astype(np.float32), "darkfield": dark.astype(np.float32), "offset": float(dark.mean())}


def coefficients(shading):
    flat = shading["flatfield"].astype(np.float64)
    dark = shading["darkfield"].astype(np.float64)
    return np.stack([1.0 / flat, shading["offset"] - dark / flat], axis=-1).astype(np.float32)


def apply(data, coeff, out_dtype=None):
    """a(y, x) * (float32)data + b(y, x) in float32, the product rounded before the sum; integer outputs rounded half to even and
    saturated, a NaN stored as 0; a float32 output keeps NaN."""
    data = np.asarray(data)
    coeff = np.asarray(coeff, dtype=np.float32)
    out_dtype = data.dtype if out_dtype is None else np.dtype(out_dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        y = ((coeff[..., 0] * data.astype(np.float32)).astype(np.float32) + coeff[..., 1]).astype(np.float32)
        if out_dtype.kind == "f":
            return y
        vmax = np.float32(np.iinfo(out_dtype).max)
        r = np.rint(y)
        r = np.where(r >= 0, r, np.float32(0))
        r = np.where(r > vmax, vmax, r)
    return r.astype(out_dtype)
