"""Thin array-level wrappers of the registration entry points of libmvs_hip.so."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._operands import dense_operand, fill_view_geometry, operand_pair, result_array, shape3, view_data, written
from .device import is_device_array

_F32 = (np.float32,)


def _crop_pair(a, b, device, names="images"):
    """The two float32 crops of one call: ``(pointer a, pointer b, mem, what keeps them alive)``."""
    return operand_pair(a, b, _F32, device, "registration kernels", host_dtype=np.float32, names=names)


def rescale_intensity(im, device=0, out_on_device=False):
    """skimage.exposure.rescale_intensity(im, in_range=(nanmin, nanmax), out_range=(0, 1)) on the GPU.
    Returns (rescaled float32, nanmin, nanmax, n_valid)."""
    lib = _lib.init(device)
    ptr, mem, keep = dense_operand(im, _F32, device, "registration kernels", host_dtype=np.float32)
    n = int(np.prod(im.shape))
    mn, mx, nv = C.c_float(), C.c_float(), C.c_int64()
    out, optr, omem = result_array(im.shape, np.float32, out_on_device, device)
    rc = lib.mvs_rescale_intensity(device, ptr, mem, n, optr, omem, C.byref(mn), C.byref(mx), C.byref(nv))
    _lib.check(rc, device, "mvs_rescale_intensity")
    return written(out), float(mn.value), float(mx.value), int(nv.value)


def phase_cross_correlation(reference_image, moving_image, upsample_factor=1, normalization="phase", device=0,
                            return_debug=False):
    """skimage.registration.phase_cross_correlation(ref, mov, upsample_factor=, normalization=,
    disambiguate=False)[0] on the GPU (NaN-free float32 inputs of equal shape)."""
    lib = _lib.init(device)
    if tuple(reference_image.shape) != tuple(moving_image.shape):
        raise ValueError("images must be same shape")
    if normalization not in ("phase", None):
        raise ValueError("normalization must be either phase or None")
    shape = tuple(int(s) for s in reference_image.shape)
    ndim = len(shape)
    p0, p1, m0, keep = _crop_pair(reference_image, moving_image, device)
    shift = (C.c_double * 3)()
    peak = (C.c_int64 * 3)()
    pabs = C.c_float()
    rc = lib.mvs_phasecorr(device, p0, p1, m0, ndim, _lib.i64x3(shape3(shape)), 1 if normalization == "phase" else 0,
                           int(upsample_factor), shift, peak, C.byref(pabs))
    _lib.check(rc, device, "mvs_phasecorr")
    s = np.array(list(shift)[3 - ndim:], dtype=np.float32)
    if return_debug:
        return s, {"peak_index": np.array(list(peak)[3 - ndim:]), "peak_abs": float(pabs.value)}
    return s


def fftn(a, inverse=False, device=0):
    """numpy.fft.fftn / ifftn (the inverse WITHOUT its 1/N) of a 2D / 3D complex64 host array on the GPU (mvs_fft_c2c)."""
    lib = _lib.init(device)
    out = np.ascontiguousarray(a, dtype=np.complex64).copy()
    rc = lib.mvs_fft_c2c(device, out.ctypes.data, _lib.MVS_MEM_HOST, out.ndim, _lib.i64x3(shape3(out.shape)), 1 if inverse else 0)
    _lib.check(rc, device, "mvs_fft_c2c")
    return out


def phase_cross_correlation_multi(reference_image, moving_image, upsample_factor=1, normalizations=("phase", None), device=0,
                                  return_refined=False):
    """``phase_cross_correlation`` for several normalisations of one image pair; the forward transforms are
    shared (mvs_phasecorr_multi).  Returns a list of (shift, debug) like ``phase_cross_correlation(return_debug=True)``.
    ``return_refined``: the same launches through mvs_phasecorr_multi_refined; ``debug["refined"]`` is then what the upsampled-DFT
    refinement computed, a complex64 array of ``ceil(1.5 * upsample_factor)`` samples per axis -- skimage's
    ``_upsampled_dft(image_product.conj(), ...)`` before its final ``.conj()`` -- or None for ``upsample_factor == 1``."""
    lib = _lib.init(device)
    if tuple(reference_image.shape) != tuple(moving_image.shape):
        raise ValueError("images must be same shape")
    for normalization in normalizations:
        if normalization not in ("phase", None):
            raise ValueError("normalization must be either phase or None")
    shape = tuple(int(s) for s in reference_image.shape)
    ndim = len(shape)
    p0, p1, m0, keep = _crop_pair(reference_image, moving_image, device)
    nn = len(normalizations)
    norms = (C.c_int32 * nn)(*[1 if v == "phase" else 0 for v in normalizations])
    shift = (C.c_double * (3 * nn))()
    peak = (C.c_int64 * (3 * nn))()
    pabs = (C.c_float * nn)()
    refined = None
    if return_refined:
        U = int(np.ceil(np.float32(upsample_factor) * np.float32(1.5)))
        if int(upsample_factor) > 1:
            refined = np.zeros((nn,) + (U,) * ndim, dtype=np.complex64)
        rc = lib.mvs_phasecorr_multi_refined(device, p0, p1, m0, ndim, _lib.i64x3(shape3(shape)), norms, nn, int(upsample_factor),
                                             shift, peak, pabs, refined.ctypes.data if refined is not None else None,
                                             2 * refined.size if refined is not None else 0)
        _lib.check(rc, device, "mvs_phasecorr_multi_refined")
    else:
        rc = lib.mvs_phasecorr_multi(device, p0, p1, m0, ndim, _lib.i64x3(shape3(shape)), norms, nn, int(upsample_factor),
                                     shift, peak, pabs)
        _lib.check(rc, device, "mvs_phasecorr_multi")
    out = []
    for i in range(nn):
        s = np.array(list(shift)[3 * i + 3 - ndim:3 * i + 3], dtype=np.float32)
        debug = {"peak_index": np.array(list(peak)[3 * i + 3 - ndim:3 * i + 3]), "peak_abs": float(pabs[i])}
        if return_refined:
            debug["refined"] = refined[i] if refined is not None else None
        out.append((s, debug))
    return out


def register_crops(im0, im1, upsample_factor, region_mode=None, constant_check=False, device=0):
    """registration.phase_correlation_registration in one library call (mvs_register_crops).  Returns
    (t (ndim,) float64, quality, status, n_candidates); status as documented in include/mvs_hip.h."""
    lib = _lib.init(device)
    shape = tuple(int(s) for s in im0.shape)
    ndim = len(shape)
    p0, p1, m0, keep = _crop_pair(im0, im1, device)
    t = (C.c_double * 3)()
    q = C.c_double()
    status = C.c_int32()
    ncand = C.c_int32()
    mode = -1 if region_mode is None else {"union": 0, "intersection": 1}[region_mode]
    rc = lib.mvs_register_crops(device, p0, p1, m0, ndim, _lib.i64x3(shape3(shape)), int(upsample_factor), mode, int(bool(constant_check)),
                                t, C.byref(q), C.byref(status), C.byref(ncand))
    _lib.check(rc, device, "mvs_register_crops")
    return np.array(list(t)[3 - ndim:], dtype=np.float64), float(q.value), int(status.value), int(ncand.value)


def register_views(data0, matrix0, offset0, data1, matrix1, offset1, out_shape, upsample_factor, region_mode=None, constant_check=False,
                   device=0):
    """Resample both overlap crops and register them in one library call (mvs_register_views).  ``data*``: DeviceArray slabs
    (strided windows allowed), ``matrix*`` (diagonal given as a list) / ``offset*``: the pixel affines of
    transformation.get_pixel_affine, ``out_shape``: the fixed view's overlap grid.  Returns like ``register_crops``."""
    lib = _lib.init(device)
    ndim = len(out_shape)
    views = (_lib.mvs_view_t * 2)()
    keep = []
    for v, data, mdiag, off in ((views[0], data0, matrix0, offset0), (views[1], data1, matrix1, offset1)):
        if not is_device_array(data) or data.dtype not in _lib.DTYPE_CODES:
            raise TypeError("register_views needs DeviceArray slabs of a supported dtype")
        ptr, s3, st3, mem, kept = view_data(data, device)
        fill_view_geometry(v, ptr, _lib.DTYPE_CODES[kept.dtype], mem, s3, st3, np.diag([float(m) for m in mdiag]), [float(o) for o in off])
        keep.append(kept)
    t = (C.c_double * 3)()
    q = C.c_double()
    status = C.c_int32()
    ncand = C.c_int32()
    mode = -1 if region_mode is None else {"union": 0, "intersection": 1}[region_mode]
    rc = lib.mvs_register_views(device, C.byref(views[0]), C.byref(views[1]), ndim, _lib.i64x3(shape3(out_shape)), int(upsample_factor), mode,
                                int(bool(constant_check)), t, C.byref(q), C.byref(status), C.byref(ncand))
    _lib.check(rc, device, "mvs_register_views")
    return np.array(list(t)[3 - ndim:], dtype=np.float64), float(q.value), int(status.value), int(ncand.value)


def score_candidates(im0, im1, t_candidates, region_mode, data_range, im1_min, device=0, quality_for_all=True):
    """The candidate loop of registration.py:493-556 on the GPU.  im0 / im1: rescaled float32 images
    (NaN = outside).  Returns (ssim, spearman, code) arrays; code 1 = (-1,-1) appended, 2 = `continue`.
    ``quality_for_all=False`` evaluates the Spearman coefficient only for the best-SSIM candidate(s) (NaN
    elsewhere) -- the only value the reference's result uses."""
    lib = _lib.init(device)
    shape = tuple(int(s) for s in im0.shape)
    ndim = len(shape)
    p0, p1, m0, keep = _crop_pair(im0, im1, device)
    t_all = np.asarray(t_candidates, dtype=np.float64).reshape(-1, ndim)
    # both phase-correlation variants usually agree, so the enumeration holds exact duplicates; scoring is a
    # pure function of t: evaluate each distinct vector once and scatter (list order / nanargmax unchanged)
    t_uniq, inverse = np.unique(t_all, axis=0, return_inverse=True)
    t = np.ascontiguousarray(t_uniq)
    inverse = np.asarray(inverse).reshape(-1)
    n = t.shape[0]
    ssim = np.empty(n, dtype=np.float64)
    spear = np.empty(n, dtype=np.float64)
    code = np.empty(n, dtype=np.int32)
    rc = lib.mvs_score_candidates(
        device, p0, p1, m0, ndim, _lib.i64x3(shape3(shape)), t.ctypes.data_as(C.POINTER(C.c_double)), n,
        {"union": 0, "intersection": 1}[region_mode], float(data_range), float(im1_min), int(bool(quality_for_all)),
        ssim.ctypes.data_as(C.POINTER(C.c_double)), spear.ctypes.data_as(C.POINTER(C.c_double)),
        code.ctypes.data_as(C.POINTER(C.c_int32)),
    )
    _lib.check(rc, device, "mvs_score_candidates")
    return ssim[inverse], spear[inverse], code[inverse]


def score_candidates_argmax(im0, im1, t_candidates, region_mode, data_range, im1_min, value_bound, device=0):
    """The candidate loop as ``register_crops`` runs it (mvs_score_candidates_argmax): only the arg max is needed, so the pruned
    search and its float32 walk may run.  ``t_candidates``: distinct rows, scored in the given order.  Returns (ssim, spearman, code,
    ssim_rounds, state): ``state`` holds the ``_lib.MVS_SCORE_*`` bits, ``ssim_rounds`` the mean SSIM of a complete candidate when
    the rounds of the search ended (NaN for the others); a dropped candidate's ``ssim`` is the bound its mean could not exceed."""
    lib = _lib.init(device)
    shape = tuple(int(s) for s in im0.shape)
    ndim = len(shape)
    p0, p1, m0, keep = _crop_pair(im0, im1, device)
    t = np.ascontiguousarray(np.asarray(t_candidates, dtype=np.float64).reshape(-1, ndim))
    n = t.shape[0]
    if len(np.unique(t, axis=0)) != n:
        raise ValueError("score_candidates_argmax: duplicate candidates")
    ssim, spear, rounds = (np.empty(n, dtype=np.float64) for _ in range(3))
    code, state = (np.empty(n, dtype=np.int32) for _ in range(2))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = lib.mvs_score_candidates_argmax(
        device, p0, p1, m0, ndim, _lib.i64x3(shape3(shape)), t.ctypes.data_as(dp), n, {"union": 0, "intersection": 1}[region_mode],
        float(data_range), float(im1_min), float(value_bound), ssim.ctypes.data_as(dp), spear.ctypes.data_as(dp), code.ctypes.data_as(ip),
        rounds.ctypes.data_as(dp), state.ctypes.data_as(ip),
    )
    _lib.check(rc, device, "mvs_score_candidates_argmax")
    return ssim, spear, code, rounds, state


def bin_mean(data, bins, device=0, wait=True, out=None):
    """``coarsen(bins, boundary="trim").mean().astype(dtype)`` (registration.py:1732-1741) on the GPU.
    ``data``: numpy array or (strided) DeviceArray, spatial dims only; ``bins``: per-axis ints.  ``wait=False`` (device
    arrays only) queues the kernel and returns: ``_lib.synchronize(device)`` before the result is used; ``out``: a contiguous
    DeviceArray of the binned shape to write into (one allocation for many tiles)."""
    lib = _lib.init(device)
    nd = data.ndim
    bins = [int(b) for b in bins]
    shape = [int(s) for s in data.shape]
    oshape = [s // b for s, b in zip(shape, bins)]
    dtype = np.dtype(data.dtype)
    if dtype not in _lib.DTYPE_CODES:
        raise TypeError(f"unsupported dtype {dtype}")
    on_dev = is_device_array(data)
    ptr, s3, st3, mem, data = view_data(data, device, wait=False)
    out, optr, omem = result_array(oshape, dtype, on_dev, device, out if on_dev else None, "bin_mean: out")
    b3 = [1] * (3 - nd) + bins
    if not wait and on_dev:
        rc = lib.mvs_bin_mean_async(device, ptr, _lib.DTYPE_CODES[dtype], _lib.i64x3(s3), _lib.i64x3(st3), _lib.i64x3(b3), optr)
        _lib.check(rc, device, "mvs_bin_mean_async")
        return written(out)
    rc = lib.mvs_bin_mean(device, ptr, _lib.DTYPE_CODES[dtype], mem, _lib.i64x3(s3), _lib.i64x3(st3), _lib.i64x3(b3), optr, omem)
    _lib.check(rc, device, "mvs_bin_mean")
    return written(out)


def _pose_geometry(fixed, moving, A, t, device):
    """The arguments the affine entry points share -- crop pointers, mem, ndim, shape, the pose ``(A, t)`` embedded into 3 x 3 / 3
    -- and the objects that keep them alive during the call."""
    shape = tuple(int(s) for s in fixed.shape)
    if tuple(moving.shape) != shape:
        raise ValueError("crops must have the same shape")
    ndim = len(shape)
    p0, p1, m0, keep = _crop_pair(fixed, moving, device, names="crops")
    A3 = np.eye(3)
    A3[3 - ndim:, 3 - ndim:] = np.asarray(A, dtype=np.float64).reshape(ndim, ndim)
    t3 = np.zeros(3)
    t3[3 - ndim:] = np.asarray(t, dtype=np.float64).reshape(ndim)
    dp = C.POINTER(C.c_double)
    return (p0, p1, m0, ndim, _lib.i64x3(shape3(shape)), A3.ctypes.data_as(dp), t3.ctypes.data_as(dp)), (keep, A3, t3)


def affine_normal_equations(fixed, moving, A, t, gain=1.0, bias=0.0, device=0):
    """Normal equations of one Gauss-Newton step of the intensity registration (mvs_affine_normal_eq).  ``fixed`` / ``moving``:
    same-shape float32 crops (NaN = outside), both numpy or both contiguous DeviceArrays; ``(A, t)``: the centred pose, fixed
    voxel x samples moving at ``c + t + A (x - c)``.  Returns (H (P, P), b (P,), sum r^2, n valid, (sum v, sum F, sum vF,
    sum v^2, sum F^2)) with P = ndim (ndim + 1) and the parameters ordered as the rows of ``[A | t]``."""
    lib = _lib.init(device)
    geom, keep = _pose_geometry(fixed, moving, A, t, device)
    ndim = geom[3]
    out = np.empty(_lib.MVS_AFFINE_NEQ_LEN, dtype=np.float64)
    rc = lib.mvs_affine_normal_eq(device, *geom, float(gain), float(bias), out.ctypes.data_as(C.POINTER(C.c_double)))
    _lib.check(rc, device, "mvs_affine_normal_eq")
    P = ndim * (ndim + 1)
    H = out[:P * P].reshape(P, P).copy()
    b = out[P * P:P * P + P].copy()
    rest = out[P * P + P:P * P + P + 7]
    return H, b, float(rest[0]), float(rest[1]), tuple(float(v) for v in rest[2:7])


def finite_range(a, device=0):
    """(minimum, maximum, count) of the finite values of a float32 crop (mvs_finite_range); NaN, NaN, 0 when it has none."""
    lib = _lib.init(device)
    ptr, mem, keep = dense_operand(a, _F32, device, "registration kernels", host_dtype=np.float32)
    mn, mx, nv = C.c_float(), C.c_float(), C.c_int64()
    rc = lib.mvs_finite_range(device, ptr, mem, int(np.prod(a.shape)), C.byref(mn), C.byref(mx), C.byref(nv))
    _lib.check(rc, device, "mvs_finite_range")
    return float(mn.value), float(mx.value), int(nv.value)


def affine_joint_hist(fixed, moving, A, t, n_bins, ranges, device=0):
    """Joint histogram of the Mattes metric over the warped crop pair (mvs_affine_joint_hist).  Crops and pose as
    ``affine_normal_equations``; ``ranges`` = (f_lo, f_scale, m_lo, m_scale).  Returns (hist (B, B) int64: rows = fixed bin,
    columns = moving bin, in units of 2^-20 sample; n valid)."""
    lib = _lib.init(device)
    geom, keep = _pose_geometry(fixed, moving, A, t, device)
    hist = np.empty((int(n_bins), int(n_bins)), dtype=np.int64)
    n = C.c_int64()
    rc = lib.mvs_affine_joint_hist(device, *geom, int(n_bins), *[float(v) for v in ranges], hist.ctypes.data_as(C.POINTER(C.c_int64)),
                                   C.byref(n))
    _lib.check(rc, device, "mvs_affine_joint_hist")
    return hist, int(n.value)


def affine_mi_gradient(fixed, moving, A, t, n_bins, ranges, table, device=0):
    """Gradient sums of the Mattes metric (mvs_affine_mi_gradient); ``table``: (B, B) L[a][b], passed as float32.  Returns
    (sums (P,) in the order of the rows of ``[A | t]``, n valid); d MI / d theta = (m_scale / n) * sums."""
    lib = _lib.init(device)
    geom, keep = _pose_geometry(fixed, moving, A, t, device)
    tab = np.ascontiguousarray(table, dtype=np.float32)
    if tab.shape != (int(n_bins), int(n_bins)):
        raise ValueError("table must be n_bins x n_bins")
    out = np.empty(_lib.MVS_AFFINE_MI_GRAD_LEN, dtype=np.float64)
    rc = lib.mvs_affine_mi_gradient(device, *geom, int(n_bins), *[float(v) for v in ranges], tab.ctypes.data_as(C.POINTER(C.c_float)),
                                    out.ctypes.data_as(C.POINTER(C.c_double)))
    _lib.check(rc, device, "mvs_affine_mi_gradient")
    P = geom[3] * (geom[3] + 1)
    return out[:P].copy(), int(out[P])
