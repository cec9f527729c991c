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
from ._stack_ops import run_stack_call, stack_dims, stack_inputs

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

    def call(shape3, t3, out_dtype_code, out_ptr, out_mem):
        opts = _lib.mvs_deconv_opts_t()
        opts.n_iterations = int(n_iterations)
        opts.erosion_px = int(erosion_px)
        opts.lambda_reg = float(lambda_reg)
        opts.min_value = float(min_value)
        opts.trim[:] = t3
        opts.out_dtype = out_dtype_code
        opts.flags = _lib.MVS_DECONV_PREPARE_WEIGHTS if prepare_weights else 0
        return lib.mvs_mv_deconv(device, C.c_void_p(views.ptr), C.c_void_p(weights.ptr), views.shape[0], _lib.i64x3(shape3), ndim,
                                 k1.ctypes.data, k2.ctypes.data, _lib.i64x3(k1.shape[1:]),
                                 None if s1 is None else s1.ctypes.data, None if s2 is None else s2.ctypes.data,
                                 C.byref(opts), C.c_void_p(out_ptr), out_mem)

    return run_stack_call("mvs_mv_deconv", views, ndim, trim, out_dtype, out_on_device, device, out, call)


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
    name = "multi_view_deconvolution"
    n_views, ndim = stack_dims(name, transformed_views, blending_weights)
    kernels = _kernels(n_views, ndim, psfs, psf_type, output_spacing, na, wavelength_um)      # (its errors come before any upload)
    views, weights, ndim, out_dtype, on_dev, cast_dtype = stack_inputs(name, transformed_views, blending_weights, device)
    res = _run(views, weights, ndim, kernels, n_iterations, lambda_reg, min_value, sample_boundary_erosion_px, [0] * ndim, out_dtype,
               on_dev, device)
    return res if cast_dtype is None else res.astype(cast_dtype, copy=False)


# ---- PSFs measured from beads --------------------------------------------------------------------------------------------------
_PSF_STATUS = {0: "used", 1: "outside", 2: "empty"}


def _psf_extents(psf_shape, sdims):
    """The window's extent per spatial dim: odd, 3 .. KERNEL_LIMIT (else ``ValueError``)."""
    if isinstance(psf_shape, dict):
        if sorted(psf_shape) != sorted(sdims):
            raise ValueError(f"psf_shape must have one entry per spatial dim {sdims}")
        shape = [psf_shape[d] for d in sdims]
    else:
        shape = list(np.atleast_1d(psf_shape))
        if len(shape) != len(sdims):
            raise ValueError(f"psf_shape must have one entry per spatial dim {sdims}")
    for n in shape:
        if int(n) != n or int(n) % 2 == 0 or not 3 <= int(n) <= KERNEL_LIMIT:
            raise ValueError(f"psf_shape {tuple(shape)}: every extent must be odd and in 3..{KERNEL_LIMIT}")
    return tuple(int(n) for n in shape)


def extract_psf(sim, points, psf_shape, affine=None, output_spacing=None, refine_iterations=1, min_correlation=None,
                max_beads=None, device=0, return_info=False):
    """The PSF of one view, measured from its beads on the OUTPUT grid of a fusion: the average of the background-subtracted,
    unit-sum windows around the beads (mvs_psf_extract, csrc/mvs_psf.hip), normalised to sum 1 -- one entry of ``psfs`` of
    ``multi_view_deconvolution``.

    ``sim``: the view (2-D / 3-D uint8 / uint16 / float32; numpy- or ``DeviceArray``-backed; the first field of its non-spatial
    dims); ``points``: (n, ndim) physical bead positions in the view's own frame, as ``detection.detect_beads`` returns them;
    ``psf_shape``: odd extents in 3..63, a tuple or a dict per dim; ``affine``: the view -> world affine (default identity; only
    its linear part enters; singular: ``ValueError``); ``output_spacing``: the fused grid's spacing (dict or sequence; default
    the view's own).  A window offset ``o`` in output voxels is sampled at ``c + M o`` in view pixels,
    ``M = diag(1 / spacing) L^-1 diag(output_spacing)``.

    Beads whose windows hold another bead's centre are dropped (``too_close``), then the first ``max_beads`` remain.  Per bead
    the background is the mean over the window's shell, the centre is refined ``refine_iterations`` times by the centroid of the
    background-subtracted window, and a bead whose window leaves the view is ``outside``, one with no signal ``empty``.  With
    ``min_correlation`` the beads whose Pearson correlation with the average is lower are dropped (``low_correlation``) and the
    rest averaged again at their refined centres.  No bead left: ``ValueError``.

    Returns the float32 PSF of ``psf_shape``; with ``return_info`` also a dict: ``centers`` (physical, refined), ``status`` (per
    given bead: ``used`` / ``outside`` / ``empty`` / ``too_close`` / ``low_correlation`` / ``skipped`` (beyond ``max_beads``)),
    ``background``, ``ncc`` (NaN where not computed), ``n_used``."""
    from . import _psf_ops, msi_utils, param_utils
    from . import spatial_image_utils as si_utils

    if msi_utils.is_msim(sim):
        sim = msi_utils.get_sim_from_msim(sim, scale="scale0")
    sim = si_utils.get_sim_field(sim)
    sdims = si_utils.get_spatial_dims_from_sim(sim)
    ndim = len(sdims)
    shape = _psf_extents(psf_shape, sdims)
    radius = [(n - 1) // 2 for n in shape]
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != ndim:
        raise ValueError(f"points must have shape (n_points, {ndim}) for this image, got {points.shape}")
    spacing = si_utils.get_spacing_from_sim(sim, asarray=True)
    origin = si_utils.get_origin_from_sim(sim, asarray=True)
    full = np.eye(ndim + 1) if affine is None else param_utils.select_time(affine, 0)
    if full.shape != (ndim + 1, ndim + 1):
        raise ValueError(f"affine must be {ndim + 1} x {ndim + 1}")
    if output_spacing is None:
        out_sp = spacing
    elif isinstance(output_spacing, dict):
        out_sp = np.array([float(output_spacing[d]) for d in sdims])
    else:
        out_sp = np.asarray(output_spacing, dtype=np.float64)
    matrix = _psf_ops.window_matrix(spacing, full[:ndim, :ndim], out_sp)
    if min_correlation is not None and not -1.0 <= float(min_correlation) <= 1.0:
        raise ValueError("min_correlation is a correlation coefficient in [-1, 1]")

    n = len(points)
    centers = (points - origin) / spacing
    status = np.array(["used"] * n, dtype=object)
    status[_psf_ops.too_close(centers, matrix, radius)] = "too_close"
    sel = np.nonzero(status == "used")[0]
    if max_beads is not None:
        status[sel[int(max_beads):]] = "skipped"
        sel = sel[:int(max_beads)]
    if len(sel) == 0:
        raise ValueError("extract_psf: no bead is left after the separation rule")
    background = np.full(n, np.nan)
    ncc = np.full(n, np.nan)
    psf, c_out, codes, stats = _psf_ops.psf_extract(sim.data, centers[sel], matrix, radius, refine_iterations, device)
    centers = centers.copy()
    centers[sel] = c_out
    for code, name in _PSF_STATUS.items():
        status[sel[codes == code]] = name
    background[sel], ncc[sel] = stats[:, 0], stats[:, 2]
    used = sel[codes == 0]
    if len(used) and min_correlation is not None:
        low = used[~(ncc[used] >= float(min_correlation))]
        if len(low):
            status[low] = "low_correlation"
            used = used[ncc[used] >= float(min_correlation)]
            if len(used):
                psf, _, codes2, stats2 = _psf_ops.psf_extract(sim.data, centers[used], matrix, radius, 0, device)
                for code, name in _PSF_STATUS.items():
                    status[used[codes2 == code]] = name
                background[used], ncc[used] = stats2[:, 0], stats2[:, 2]
                used = used[codes2 == 0]
    if len(used) == 0:
        counts = {k: int(np.sum(status == k)) for k in sorted(set(status))}
        raise ValueError(f"extract_psf: no usable bead ({counts})")
    psf = _norm(psf)
    if not return_info:
        return psf
    return psf, {"centers": origin + centers * spacing, "status": [str(v) for v in status], "background": background, "ncc": ncc,
                 "n_used": int(len(used))}


def extract_psfs(msims, transform_key, psf_shape, points_key="beads", output_spacing=None, **kw):
    """One measured PSF per view, for ``fuse(..., fusion_func=multi_view_deconvolution, fusion_func_kwargs={"psfs": psfs})``.

    ``msims``: the views with their beads attached (``msi_utils.set_point_set`` under ``points_key``) and registered under
    ``transform_key`` (its affine at the first time point is used).  ``output_spacing`` (dict per dim): the fused grid's spacing;
    default: the spacing ``fusion.process_output_stack_properties`` gives these views, i.e. that of a default ``fuse()``.
    Remaining keywords go to ``extract_psf``."""
    from . import fusion, msi_utils
    from . import spatial_image_utils as si_utils

    if kw.get("return_info"):
        raise TypeError("extract_psfs returns the PSFs only; call extract_psf per view for the per-bead information")
    sims = [msi_utils.get_sim_from_msim(m, scale="scale0") if msi_utils.is_msim(m) else m for m in msims]
    if output_spacing is None:
        output_spacing = fusion.process_output_stack_properties(sims, transform_key=transform_key)["spacing"]
    psfs = []
    for msim, sim in zip(msims, sims):
        points = msi_utils.get_point_set(msim, points_key) if msi_utils.is_msim(msim) else si_utils.get_point_set(sim, points_key)
        psfs.append(extract_psf(sim, points, psf_shape, affine=si_utils.get_affine_from_sim(sim, transform_key),
                                output_spacing=output_spacing, **kw))
    return psfs


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
