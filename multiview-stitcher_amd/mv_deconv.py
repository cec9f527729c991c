"""Multi-view deconvolution fusion on the HIP backend (mirror of the reference's ``fusion/mv_deconv.py``).

``multi_view_deconvolution`` == fusion.multi_view_deconvolution (mv_deconv.py:251-501): Richardson-Lucy with one
compound back-projection kernel per view (Preibisch et al., Nature Methods 11, 645-648, 2014), sequential per-view
updates.  The PSFs and compound kernels are tiny host arrays built with numpy / scipy here (cached per PSF inputs,
so a chunked ``fuse()`` builds them once); every iteration runs on the GPU behind ``mvs_mv_deconv``
(csrc/mvs_deconv.hip).  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes as C
import threading
from enum import Enum

import numpy as np
from scipy import ndimage

from . import _lib
from .device import DeviceArray, is_device_array

KERNEL_LIMIT = 63          # largest kernel extent per axis of the direct convolution (csrc/mvs_deconv.hip)
SEPARABLE_TOL = 1e-6       # rank-1 test: max |K - outer(marginals)| <= SEPARABLE_TOL * max |K|


class PSFType(str, Enum):
    """Compound back-projection kernel of a view (mv_deconv.py:24-54)."""

    EFFICIENT_BAYESIAN = "EFFICIENT_BAYESIAN"   # normalise(flip(P_v) * prod_{w != v} flip(P_v) * P_w * flip(P_w))
    OPTIMIZATION_I = "OPTIMIZATION_I"           # flip(normalise(P_v * prod_{w != v} flip(P_v) * P_w))
    OPTIMIZATION_II = "OPTIMIZATION_II"         # flip(normalise(P_v ** n_views))
    INDEPENDENT = "INDEPENDENT"                 # flip(P_v): plain Richardson-Lucy per view


def _norm(kernel):
    """Scale to unit sum in float64 (when the sum is positive), return float32 (mv_deconv.py:85-91)."""
    k = np.asarray(kernel, dtype=np.float64)
    total = k.sum()
    return (k / total if total > 0 else k).astype(np.float32)


def make_gaussian_psf(sigma, ndim=None, shape=None):
    """Normalised Gaussian PSF (mv_deconv.py:98-129): ``sigma`` in pixels (scalar with ``ndim``, or one per axis);
    ``shape`` defaults to ceil(6 sigma) made odd.  The kernel is gaussian_filter of a centred delta."""
    sig = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    if sig.size == 1 and ndim is not None:
        sig = np.full(int(ndim), float(sig[0]))
    if shape is None:
        shape = tuple(int(np.ceil(6.0 * s)) | 1 for s in sig)
    delta = np.zeros(tuple(shape), dtype=np.float32)
    delta[tuple(n // 2 for n in shape)] = 1.0
    return _norm(ndimage.gaussian_filter(delta, sigma=sig.tolist()))


def estimate_psf(spacing, na=0.8, wavelength_um=0.5):
    """Gaussian PSF from the pixel spacing (dict per dim) and the objective (mv_deconv.py:132-167): sigma 0.5 lambda / NA
    laterally, 2 lambda / NA^2 along z, converted to pixels, at least half a pixel."""
    lateral = 0.5 * wavelength_um / na
    axial = 2.0 * wavelength_um / (na ** 2)
    sig = [max(0.5, (axial if dim == "z" else lateral) / float(sp)) for dim, sp in spacing.items()]
    return make_gaussian_psf(sig)


def _convolve0(a, b):
    return ndimage.convolve(a, b, mode="constant", cval=0.0)


def compound_kernel(v, psfs, psf_type=PSFType.EFFICIENT_BAYESIAN):
    """Back-projection kernel of view ``v`` from the (equal-shaped, normalised) PSFs of all views
    (mv_deconv.py:172-247); products in float64, result normalised to float32."""
    kind = psf_type.value if isinstance(psf_type, PSFType) else str(psf_type)
    p = np.asarray(psfs[v], dtype=np.float64)
    pf = np.flip(p)
    if len(psfs) == 1 or kind == PSFType.INDEPENDENT.value:
        return _norm(pf)
    if kind == PSFType.OPTIMIZATION_II.value:
        return _norm(np.flip(p ** len(psfs)))
    if kind == PSFType.OPTIMIZATION_I.value:
        prod = p.copy()
        for w, q in enumerate(psfs):
            if w != v:
                prod = prod * _convolve0(pf, np.asarray(q, dtype=np.float64))
        return _norm(np.flip(prod))
    prod = pf.copy()                     # EFFICIENT_BAYESIAN (and any other name, as the reference)
    for w, q in enumerate(psfs):
        if w != v:
            q = np.asarray(q, dtype=np.float64)
            prod = prod * _convolve0(_convolve0(pf, q), np.flip(q))
    return _norm(prod)


def separable_factors(kernel, tol=SEPARABLE_TOL):
    """1-D factors (one per axis, in axis order) whose outer product is ``kernel`` when it is rank 1 -- every marginal
    (sum over the other axes) scaled so that their product reproduces K within ``tol`` * max|K| -- else None."""
    k = np.asarray(kernel, dtype=np.float64)
    total = k.sum()
    if k.ndim < 1 or total == 0 or not np.isfinite(total):
        return None
    axes = range(k.ndim)
    factors = [k.sum(axis=tuple(a for a in axes if a != d)) for d in axes]
    factors = [f / total for f in factors[:-1]] + [factors[-1]]
    outer = factors[0]
    for f in factors[1:]:
        outer = np.multiply.outer(outer, f)
    if np.abs(outer - k).max() > tol * np.abs(k).max():
        return None
    return [f.astype(np.float32) for f in factors]


_CACHE = {}
_CACHE_CAP = 32
_CACHE_LOCK = threading.Lock()


def _psf_key(psfs):
    if psfs is None:
        return None
    return tuple((np.asarray(p).dtype.str, np.asarray(p).shape, np.ascontiguousarray(p).tobytes()) for p in psfs)


def _kernels(n_views, ndim, psfs, psf_type, output_spacing, na, wavelength_um):
    """(kernels1, kernels2, sep1, sep2) as contiguous float32 stacks (V, kz, ky, kx) and separable factor tables
    (V, kz + ky + kx) or None; cached per PSF inputs (mv_deconv.py:357-404)."""
    kind = psf_type.value if isinstance(psf_type, PSFType) else str(psf_type)
    sp = None if output_spacing is None else tuple((d, float(s)) for d, s in dict(output_spacing).items())
    key = (_psf_key(psfs), kind, int(n_views), int(ndim), sp if psfs is None else None, float(na), float(wavelength_um))
    with _CACHE_LOCK:
        hit = _CACHE.get(key)
    if hit is not None:
        return hit
    if psfs is None:
        p0 = estimate_psf(dict(output_spacing), na=na, wavelength_um=wavelength_um) if output_spacing is not None \
            else make_gaussian_psf(1.5, ndim=ndim)
        base = [p0] * n_views
    else:
        if len(psfs) != n_views:
            raise ValueError(f"len(psfs) = {len(psfs)}, but n_views = {n_views}. Provide one PSF per view.")
        base = [_norm(np.asarray(p).astype(np.float32)) for p in psfs]
    if any(p.ndim != ndim for p in base):
        raise ValueError(f"every PSF must have {ndim} dimensions (the spatial dimensions of the views)")
    big = tuple(max(p.shape[d] for p in base) for d in range(ndim))
    if max(big) > KERNEL_LIMIT:
        raise NotImplementedError(f"multi_view_deconvolution: kernel shape {big} exceeds the limit of {KERNEL_LIMIT} "
                                  "per axis of the direct convolution on the GPU")
    k1 = []
    for p in base:
        if p.shape != big:
            p = np.pad(p, [((t - a) // 2, (t - a) - (t - a) // 2) for a, t in zip(p.shape, big)], mode="constant")
        k1.append(_norm(p))
    k2 = [compound_kernel(v, k1, kind) for v in range(n_views)]
    shape3 = (1,) * (3 - ndim) + big

    def stack(ks):
        return np.ascontiguousarray(np.stack([k.reshape(shape3) for k in ks]), dtype=np.float32)

    def seps(ks):
        f = [separable_factors(k.reshape(shape3)) for k in ks]
        return None if any(x is None for x in f) else np.ascontiguousarray(np.stack([np.concatenate(x) for x in f]), dtype=np.float32)

    s1, s2 = seps(k1), seps(k2)
    out = (stack(k1), stack(k2), s1 if s2 is not None else None, s2 if s1 is not None else None)
    with _CACHE_LOCK:
        if len(_CACHE) >= _CACHE_CAP:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = out
    return out


def _run(views, weights, ndim, kernels, n_iterations, lambda_reg, min_value, erosion_px, trim, out_dtype, out_on_device, device,
         prepare_weights=False, out=None):
    """mvs_mv_deconv on device float32 stacks (V, *S): the deconvolved chunk, trimmed by ``trim`` (per spatial axis),
    nan_to_num'd and cast to ``out_dtype``; a DeviceArray or a numpy array.  ``prepare_weights``: ``weights`` holds raw
    blending weights, masked by the views' coverage and normalised in place on the device first.  ``out``: a contiguous
    DeviceArray of the result shape and dtype to write into (with ``out_on_device``)."""
    k1, k2, s1, s2 = kernels
    lib = _lib.init(device)
    n_views = views.shape[0]
    shape = (1,) * (3 - ndim) + tuple(views.shape[1:])
    t3 = [0] * (3 - ndim) + [int(t) for t in trim]
    res_shape = tuple(s - 2 * t for s, t in zip(views.shape[1:], trim))
    opts = _lib.mvs_deconv_opts_t()
    opts.n_iterations = int(n_iterations)
    opts.erosion_px = int(erosion_px)
    opts.lambda_reg = float(lambda_reg)
    opts.min_value = float(min_value)
    for k in range(3):
        opts.trim[k] = t3[k]
    opts.out_dtype = _lib.DTYPE_CODES[np.dtype(out_dtype)]
    opts.flags = _lib.MVS_DECONV_PREPARE_WEIGHTS if prepare_weights else 0
    if out_on_device:
        if out is None:
            out = DeviceArray.empty(res_shape, out_dtype, device)
        elif tuple(out.shape) != res_shape or not out.is_contiguous() or out.dtype != np.dtype(out_dtype):
            raise ValueError("out must be a contiguous DeviceArray of the result shape and dtype")
        optr, omem = out.ptr, _lib.MVS_MEM_DEVICE
    else:
        out = np.empty(res_shape, dtype=out_dtype)
        optr, omem = out.ctypes.data, _lib.MVS_MEM_HOST
    rc = lib.mvs_mv_deconv(device, C.c_void_p(views.ptr), C.c_void_p(weights.ptr), n_views, _lib.i64x3(shape), ndim,
                           k1.ctypes.data, k2.ctypes.data, _lib.i64x3(k1.shape[1:]),
                           None if s1 is None else s1.ctypes.data, None if s2 is None else s2.ctypes.data,
                           C.byref(opts), C.c_void_p(optr), omem)
    _lib.check(rc, device, "mvs_mv_deconv")
    if out_on_device:
        out.mark_written()
    return out


def multi_view_deconvolution(
    transformed_views,
    blending_weights,
    psfs=None,
    psf_type=PSFType.EFFICIENT_BAYESIAN,
    n_iterations=10,
    lambda_reg=0.0,
    min_value=1e-4,
    output_spacing=None,
    na=0.8,
    wavelength_um=0.5,
    sample_boundary_erosion_px=0,
    device=0,
):
    """fusion.multi_view_deconvolution (mv_deconv.py:251-501) on the GPU.

    ``transformed_views`` / ``blending_weights``: (n_views, [z,] y, x), NaN in a view = outside it, weights normalised.
    numpy inputs return numpy in the views' dtype; ``DeviceArray`` inputs (float32, contiguous) return a ``DeviceArray``
    without a host round trip.  ``psfs``: one PSF per view (else ``ValueError``), zero-padded to a common shape; without
    them the PSF is estimated from ``output_spacing`` (``na``, ``wavelength_um``) or is a 1.5-pixel Gaussian.  Kernels
    larger than 63 along an axis raise ``NotImplementedError``."""
    on_dev = is_device_array(transformed_views)
    n_views = int(transformed_views.shape[0])
    ndim = len(transformed_views.shape) - 1
    if ndim not in (2, 3):
        raise ValueError("multi_view_deconvolution fuses 2D or 3D views: transformed_views is (n_views, [z,] y, x)")
    if tuple(blending_weights.shape) != tuple(transformed_views.shape):
        raise ValueError("blending_weights must have the shape of transformed_views")
    kernels = _kernels(n_views, ndim, psfs, psf_type, output_spacing, na, wavelength_um)
    if on_dev:
        if not is_device_array(blending_weights):
            blending_weights = DeviceArray.from_host(np.ascontiguousarray(blending_weights, dtype=np.float32), device)
        for a in (transformed_views, blending_weights):
            if a.dtype != np.float32 or not a.is_contiguous():
                raise TypeError("device inputs of multi_view_deconvolution are contiguous float32 DeviceArrays")
            a.wait_ready(device)
        return _run(transformed_views, blending_weights, ndim, kernels, n_iterations, lambda_reg, min_value,
                    sample_boundary_erosion_px, [0] * ndim, np.float32, True, device)
    host = np.asarray(transformed_views)
    in_dtype = host.dtype
    views = DeviceArray.from_host(np.ascontiguousarray(host, dtype=np.float32), device)
    weights = DeviceArray.from_host(np.ascontiguousarray(blending_weights, dtype=np.float32), device)
    out_dtype = in_dtype if in_dtype in _lib.DTYPE_CODES else np.dtype(np.float32)
    res = _run(views, weights, ndim, kernels, n_iterations, lambda_reg, min_value, sample_boundary_erosion_px,
               [0] * ndim, out_dtype, False, device)
    return res.astype(in_dtype, copy=False)


def _required_overlap(func_kwargs):
    """Chunk halo for the deconvolution (mv_deconv.py:504-527): half the estimated PSF's largest extent when
    ``output_spacing`` is among the kwargs, else 4 (the 1.5-pixel default PSF of 9 pixels)."""
    kwargs = func_kwargs or {}
    if kwargs.get("output_spacing") is not None:
        psf = estimate_psf(kwargs["output_spacing"], na=kwargs.get("na", 0.8), wavelength_um=kwargs.get("wavelength_um", 0.5))
        size = max(psf.shape)
    else:
        size = int(np.ceil(6.0 * 1.5)) | 1
    return size // 2


multi_view_deconvolution.required_overlap = _required_overlap
