"""Pairwise registration on the HIP backend (mirror of the reference's ``registration`` API for the hot path).

``phase_correlation_registration`` == registration.phase_correlation_registration
    (src/multiview_stitcher/registration.py:353-565): the host keeps the reference's control flow
    (candidate enumeration, quirks Q1-Q3, nanargmax) and every voxel-sized step runs in
    libmvs_hip.so: mvs_rescale_intensity, mvs_phasecorr, mvs_score_candidates.
"""

from __future__ import annotations

import collections
import ctypes as C
import logging
import os
import warnings

import threading

import numpy as np

from . import _lib, _reg_ops, msi_utils, param_utils
from . import spatial_image_utils as si_utils
from .device import is_device_array

logger = logging.getLogger(__name__)


def _as_array(x):
    return x.data if hasattr(x, "dims") and hasattr(x, "coords") else x


def _enumerate_candidates(shift_candidates, shape, ndim):
    """registration.py:453-477: per shift estimate and per axis with a non-zero shift the four variants
    {s, -s, -(s - N), -s - N}; keep |t| < max over ALL dims of the image shape.  Same order as the reference's
    nested loops (itertools.product over the axes, last axis fastest); plain Python floats, no per-element numpy calls."""
    import itertools

    max_shift_per_dim = float(max(shape))
    t_candidates = []
    for shift_candidate in shift_candidates:
        per_axis = []
        for d in range(ndim):
            sc = shift_candidate[d]
            if sc == 0:
                per_axis.append((sc,))
            else:
                n = shape[d]
                per_axis.append((sc, -sc, -(sc - n), -sc - n))
        for t in itertools.product(*per_axis):
            if max(abs(v) for v in t) < max_shift_per_dim:
                t_candidates.append(list(t))
    return t_candidates


def _default_upsample_factor(ndim):
    """``upsample_factor`` of the phase correlation when the caller gives none (registration.py:410-411)."""
    return 10 if ndim == 2 else 2


def phase_correlation_registration(fixed_data, moving_data, disambiguate_region_mode=None, device=0,
                                   return_debug=False, _constant_check=False, **skimage_phase_corr_kwargs):
    """Translation between two same-shape overlap crops (float32, NaN = outside the view).

    Returns ``{"affine_matrix": (ndim+1, ndim+1) translation mapping fixed px -> moving px,
    "quality": float}`` exactly like the reference, including its ``[zeros(ndim)]`` return when no
    candidate survives (registration.py:479-480)."""
    im0 = _as_array(fixed_data)
    im1 = _as_array(moving_data)
    if tuple(im0.shape) != tuple(im1.shape):
        raise ValueError("fixed and moving crops must have the same shape")
    shape = tuple(int(s) for s in im0.shape)
    ndim = len(shape)
    on_dev = is_device_array(im0)

    if not return_debug and set(skimage_phase_corr_kwargs) <= {"upsample_factor"}:
        # the whole function as one library call (same steps, same quirks); the Python flow below stays for the debug
        # outputs and for callers that pass other phase_cross_correlation keywords
        uf = skimage_phase_corr_kwargs.get("upsample_factor", _default_upsample_factor(ndim))
        t, quality, status, _ = _reg_ops.register_crops(im0, im1, uf, disambiguate_region_mode, _constant_check, device)
        if status == 2:
            warnings.warn(
                "An overlap region between tiles/views is all zero or constant. Assuming identity transform.",
                UserWarning, stacklevel=3,
            )
            return {"affine_matrix": param_utils.identity_transform(ndim), "quality": np.nan}
        if status == 1:
            return [np.zeros(ndim)]
        if status == 3:
            raise ValueError("All-NaN slice encountered")     # what np.nanargmax raises in the reference (registration.py:558-559)
        return {"affine_matrix": param_utils.affine_from_translation([float(v) for v in t]), "quality": quality}

    # normalise (registration.py:381-389); the kernel also reports nanmin/nanmax/#valid of the INPUT
    im0, min0, max0, nvalid0 = _reg_ops.rescale_intensity(im0, device, out_on_device=on_dev)
    im1, min1, max1, nvalid1 = _reg_ops.rescale_intensity(im1, device, out_on_device=on_dev)
    if _constant_check and (min0 == max0 or min1 == max1):
        # dispatch_pairwise_reg_func's guard (registration.py:1500-1520), folded in here so that the
        # nanmin / nanmax pass over both crops is not run twice
        warnings.warn(
            "An overlap region between tiles/views is all zero or constant. Assuming identity transform.",
            UserWarning, stacklevel=3,
        )
        return {"affine_matrix": param_utils.identity_transform(ndim), "quality": np.nan}
    n = int(np.prod(shape))
    has_nan = (nvalid0 < n) or (nvalid1 < n)
    if disambiguate_region_mode is None:
        disambiguate_region_mode = "intersection" if has_nan else "union"
    if "upsample_factor" not in skimage_phase_corr_kwargs:
        skimage_phase_corr_kwargs["upsample_factor"] = _default_upsample_factor(ndim)
    upsample_factor = skimage_phase_corr_kwargs["upsample_factor"]

    # strategy of the reference: phase correlation with and without normalisation, the candidate with
    # the best structural similarity wins (registration.py:413-431). NaNs -> 0 happens in the kernel.
    shift_candidates, pcc_debug = [], []
    for s, dbg in _reg_ops.phase_cross_correlation_multi(im0, im1, upsample_factor, ("phase", None), device):
        shift_candidates.append(s)
        pcc_debug.append(dbg)
    if has_nan:
        # the masked variant is called with inverted masks on NaN-holding images (registration.py:433-443)
        # and yields a zero shift: it only adds the candidate t = 0
        shift_candidates.append(np.zeros(ndim, dtype=np.float32))

    # after rescaling, the values present are exactly min -> 0 and max -> 1 per image
    def _rescaled_range(mn, mx, nv):
        if nv == 0:
            return np.nan, np.nan
        return (0.0, 1.0) if mx != mn else (float(np.float32(mn)), float(np.float32(mn)))

    lo0, hi0 = _rescaled_range(min0, max0, nvalid0)
    lo1, hi1 = _rescaled_range(min1, max1, nvalid1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        data_range = np.float32(np.nanmax([hi0, hi1])) - np.float32(np.nanmin([lo0, lo1]))
    im1_min = lo1

    t_candidates = _enumerate_candidates(shift_candidates, shape, ndim)
    if not len(t_candidates):
        return [np.zeros(ndim)]

    # only the Spearman value of the winning candidate is reported, so it is only evaluated for that one
    # (all of them when the debug lists are requested)
    ssim, spear, codes = _reg_ops.score_candidates(im0, im1, t_candidates, disambiguate_region_mode, data_range, im1_min,
                                                   device, quality_for_all=return_debug)
    # metric lists exactly as the reference builds them: code 2 (`continue`, registration.py:530-533) appends nothing
    disambiguate_metric_vals = [float(ssim[i]) for i in range(len(codes)) if codes[i] != 2]
    quality_metric_vals = [float(spear[i]) for i in range(len(codes)) if codes[i] != 2]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        argmax_index = int(np.nanargmax(disambiguate_metric_vals))
    t = t_candidates[argmax_index]
    reg_result = {
        "affine_matrix": param_utils.affine_from_translation([float(v) for v in t]),
        "quality": quality_metric_vals[argmax_index],
    }
    if return_debug:
        reg_result["debug"] = {
            "shift_candidates": [np.asarray(s, dtype=np.float64) for s in shift_candidates], "pcc": pcc_debug,
            "t_candidates": np.asarray(t_candidates, dtype=np.float64), "codes": list(codes),
            "ssim": disambiguate_metric_vals, "spearman": quality_metric_vals, "argmax_index": argmax_index,
            "region_mode": disambiguate_region_mode, "data_range": float(data_range), "im1_min": float(im1_min),
        }
    return reg_result


def affine_registration(fixed_data, moving_data, transform_type="rigid", shrink_factors=(2, 1), max_iterations=(30, 20), tolerance=1e-3,
                        initial_affine="phase_correlation", fit_intensity=True, device=0, return_debug=False, metric="ssd", n_bins=32):
    """Rigid / affine intensity registration of two same-shape overlap crops (float32, NaN = outside the view): a drop-in
    ``pairwise_reg_func`` in the seat of the reference's ``registration_ANTsPy`` (registration.py:2774-2922).

    Gauss-Newton on the squared residual ``gain * moving(p(x)) + bias - fixed(x)`` (order-1 interpolation and its analytic
    gradient), coarse to fine over ``shrink_factors`` with at most ``max_iterations`` steps per level; a level ends when no
    crop corner moves by ``tolerance`` (full-resolution px) any more.  ``transform_type``: "translation", "rigid",
    "similarity" or "affine".  ``initial_affine``: "phase_correlation" (the translation ``phase_correlation_registration``
    finds), "identity" or an (ndim + 1)^2 matrix.  ``fit_intensity``: gain and bias follow the least-squares fit of the
    previous iteration's samples (else 1, 0).  Every iteration is one ``mvs_affine_normal_eq`` launch over the level's crop;
    the model algebra runs on the host in float64 (``_affine_reg``).

    Returns ``{"affine_matrix": fixed px -> moving px, "quality": masked Spearman coefficient of the aligned crops}``;
    ``return_debug`` adds ``"debug": {"history": [{level, msd, n, gain, bias, step}, ...], "initial_affine"}``.  Warns and
    returns the initial pose with quality NaN when fewer than 4 valid samples per model parameter remain or the projected
    normal equations are not positive definite.

    ``metric="mattes"`` maximises the Mattes mutual information of the two crops instead (``n_bins`` bins per axis, 8..64; an
    order-0 window on the fixed values, a cubic B-spline window on the moving ones): for crops whose intensities are not
    linearly related, such as opposite views or two channels.  Preconditioned gradient ascent with a backtracking step
    length; per iteration one ``mvs_affine_mi_gradient`` launch and one ``mvs_affine_joint_hist`` launch per tried step.
    ``fit_intensity`` is not used, and the phase-correlation start assumes related intensities too: where it cannot be trusted
    pass ``initial_affine="identity"`` (or a matrix).  ``quality`` is then the symmetric uncertainty ``2 MI / (H_F + H_M)`` of the final
    full-resolution histogram, in [0, 1], and the history rows are ``{level, mi, n, alpha, step}``.  It also warns and returns
    the initial pose when a crop is constant."""
    from . import _affine_reg

    return _affine_reg.affine_registration(fixed_data, moving_data, transform_type, shrink_factors, max_iterations, tolerance,
                                           initial_affine, fit_intensity, device, return_debug, metric, n_bins)


def masked_correlation_registration(fixed_data, moving_data, fixed_mask=None, moving_mask=None, valid_above=None, overlap_ratio=0.3,
                                    min_overlap=None, max_shift=None, subpixel=True, device=0, return_debug=False):
    """Translation between two same-shape overlap crops (float32, NaN = outside the view) by masked normalised cross-correlation
    (Padfield 2012; ``skimage.registration.phase_cross_correlation`` with ``reference_mask`` / ``moving_mask``): a drop-in
    ``pairwise_reg_func`` for overlaps that are not boxes (rotated or opposite views, whose zero-filled wedges mislead the plain
    phase correlation) and for sparse samples on a dark or structured background.

    A voxel counts when it is finite, its mask (``fixed_mask`` / ``moving_mask``: arrays of the crops' shape, non-zero = data) is
    set, and it exceeds ``valid_above`` (a scalar, or a ``(fixed, moving)`` pair; e.g. ``masks.otsu_threshold(tiles)`` through
    ``pairwise_reg_func_kwargs``).  For every integer shift ``s`` with ``|s_d| <= max_shift_d`` (a scalar or one value per axis, in
    px; default ``n_d - 1``) the Pearson correlation ``r(s)`` of ``fixed(x)`` and ``moving(x + s)`` is taken over the voxels that
    count in both; the result is the shift with the largest ``r`` among those whose overlap ``N(s)`` is at least
    ``max(overlap_ratio * max N, min_overlap)`` (``min_overlap`` defaults to ``4 ** ndim``).  Tiny overlaps correlate perfectly by
    chance: that is what the overlap rule is for.  One ``mvs_masked_corr`` call: three forward and three inverse transforms of the
    crops zero-padded to powers of two ``>= n_d + max_shift_d``; more than 2^28 padded voxels raise ``NotImplementedError`` (pass a
    smaller ``max_shift``).  ``subpixel`` refines every axis by the vertex of the parabola through ``r`` at the peak and its two
    neighbours (host, float64, clamped to half a px), on an axis only when both neighbours lie in the window, have enough overlap
    and the curvature is negative.

    Returns ``{"affine_matrix": translation mapping fixed px -> moving px, "quality": r at the integer peak, in [-1, 1]}``.  The
    quality is the quantity that was maximised and costs no further pass over the crops; the other pair functions report a masked
    Spearman coefficient of the aligned crops instead, so qualities of different pair functions are not on one scale.
    ``return_debug`` adds ``"debug": {"r", "n"`` (the window volumes, shape ``2 max_shift + 1``), ``"peak", "n_peak", "n_max",
    "n_valid", "padded_shape", "max_shift", "status", "subpixel"}``.  Warns and returns the identity with quality NaN when a crop has
    fewer than ``min_overlap`` valid voxels, is constant on them, or no shift qualifies."""
    from . import _masked_corr_ops as ops

    im0, im1 = _as_array(fixed_data), _as_array(moving_data)
    ndim = len(im0.shape)
    thr = (valid_above, valid_above) if valid_above is None or np.isscalar(valid_above) else tuple(valid_above)
    if len(thr) != 2:
        raise ValueError("valid_above is a scalar or a (fixed, moving) pair")
    res = ops.masked_corr(im0, im1, None if fixed_mask is None else _as_array(fixed_mask), None if moving_mask is None else _as_array(moving_mask),
                          thr, overlap_ratio, 4 ** ndim if min_overlap is None else min_overlap, max_shift, device, want_volumes=return_debug)
    delta = [0.0] * ndim
    if res["status"] != _lib.MVS_MASKED_CORR_OK:
        warnings.warn(f"Masked correlation: {ops.STATUS_MESSAGES[res['status']]}. Assuming identity transform.", UserWarning, stacklevel=2)
        out = {"affine_matrix": param_utils.identity_transform(ndim), "quality": np.nan}
    else:
        if subpixel:
            delta = [ops.subpixel_offset(res["r"], res["neighbour_r"][2 * d], res["neighbour_r"][2 * d + 1], res["neighbour_ok"][2 * d],
                                         res["neighbour_ok"][2 * d + 1]) for d in range(ndim)]
        out = {"affine_matrix": param_utils.affine_from_translation([float(p) + dl for p, dl in zip(res["peak"], delta)]), "quality": res["r"]}
    if return_debug:
        out["debug"] = {"r": res["r_volume"], "n": res["n_volume"], "peak": res["peak"], "n_peak": res["n_peak"], "n_max": res["n_max"],
                        "n_valid": res["n_valid"], "padded_shape": res["padded_shape"], "max_shift": res["max_shift"], "status": res["status"],
                        "subpixel": delta}
    return out


def registration_marker_based(fixed_points, moving_points, transform_type="rigid", num_neighbors=3, redundancy=1, descriptor_ratio=3.0,
                              descriptor_distance_threshold=None, descriptor_threshold_scale=1.0, ransac_max_error=5.0,
                              ransac_min_inlier_ratio=0.1, ransac_min_inlier_factor=3.0, ransac_num_iterations=1000, icp=False,
                              icp_max_error=None, icp_num_iterations=50, icp_tolerance=1e-6, random_state=0, fail_on_error=True, device=0):
    """Marker-based registration of two point sets (registration.registration_marker_based, registration.py:1165-1379; after
    BigStitcher's RGLDM bead matching): local geometric descriptors of ``fixed_points`` and ``moving_points`` ((n, ndim) arrays,
    ndim 2 or 3) are matched, inconsistent matches are removed by RANSAC, and the result is ``{"affine_matrix": fixed ->
    moving, "quality"}``.  A ``pairwise_reg_func`` for ``register``: it takes the ``fixed_points`` / ``moving_points`` that
    ``register_pair_of_msims`` reads from the views' point sets (``msi_utils.set_point_set``, e.g. what
    ``detection.detect_beads`` returns).

    Parameters and defaults are the reference's.  ``transform_type``: "translation", "rigid" or "affine".  Every point gets
    one descriptor per ``num_neighbors``-subset of its ``num_neighbors + redundancy`` nearest points: the sorted distances
    among the point and the subset.  A fixed descriptor proposes a correspondence when its nearest moving descriptor is closer
    than ``descriptor_distance_threshold`` (None: the median nearest-neighbour distance of the points times
    sqrt(descriptor length) times ``descriptor_threshold_scale``) and ``descriptor_ratio`` times closer than the nearest
    descriptor of any other moving point.  RANSAC fits minimal samples of the proposals (all combinations when there are at
    most ``ransac_num_iterations``, else that many draws from ``np.random.default_rng(random_state)``), counts the proposals
    within ``ransac_max_error``, refits on the best model's inliers and fails below ``ransac_min_inlier_ratio`` or
    ``round(minimal sample size * ransac_min_inlier_factor)`` inliers.  ``icp``: nearest-neighbour ICP refinement within
    ``icp_max_error`` (None: ``ransac_max_error``), at most ``icp_num_iterations`` iterations, until the matrix changes by
    at most ``icp_tolerance`` (Frobenius).  ``fail_on_error``: raise ValueError on failure, else warn and return identity with
    ``quality = nan``.

    The nearest-neighbour queries (mvs_knn), the descriptor vectors (mvs_marker_descriptors) and the scoring of all RANSAC
    hypotheses (mvs_marker_score) run on ``device``; arguments are validated before the device is touched.  The kernels
    take ``num_neighbors <= 5`` and at most 15 descriptors per point; beyond that NotImplementedError names the parameter.
    ``rigid`` is Umeyama's fit without scale, ``affine`` the least-squares estimator of ``param_resolution``."""
    from . import _marker_reg

    return _marker_reg.registration_marker_based(
        fixed_points, moving_points, fail_on_error=fail_on_error, transform_type=transform_type, num_neighbors=num_neighbors,
        redundancy=redundancy, descriptor_ratio=descriptor_ratio, descriptor_distance_threshold=descriptor_distance_threshold,
        descriptor_threshold_scale=descriptor_threshold_scale, ransac_max_error=ransac_max_error,
        ransac_min_inlier_ratio=ransac_min_inlier_ratio, ransac_min_inlier_factor=ransac_min_inlier_factor,
        ransac_num_iterations=ransac_num_iterations, icp=icp, icp_max_error=icp_max_error, icp_num_iterations=icp_num_iterations,
        icp_tolerance=icp_tolerance, random_state=random_state, device=device)


def _marker_registration_details(fixed_points, moving_points, **kwargs):
    """``registration_marker_based`` with its intermediate results (tests, tools): the result dict plus ``candidate_pairs``,
    ``inlier_mask`` and ``descriptor_distance_threshold``; raises ValueError on every failure."""
    from . import _marker_reg

    return _marker_reg.register_details(fixed_points, moving_points, **kwargs)


def get_optimal_registration_binning(sim1, sim2, max_total_pixels_per_stack=400**3, overlap_tolerance=None):
    """registration.get_optimal_registration_binning (registration.py:114-191): +1 steps (not doublings) on
    the axis with the smallest current spacing (z alone, or x and y together) until the larger of the two
    stacks has fewer than 400^3 voxels."""
    from . import spatial_image_utils as si_utils

    if overlap_tolerance is not None:
        raise NotImplementedError("overlap_tolerance")
    sdims = si_utils.get_spatial_dims_from_sim(sim1)
    ndim = len(sdims)
    input_spacings = [si_utils.get_spacing_from_sim(s) for s in [sim1, sim2]]
    sh1, sh2 = si_utils.get_shape_from_sim(sim1), si_utils.get_shape_from_sim(sim2)
    # a pure function of shapes and spacings: the pairs of a regular mosaic all share one answer
    memo_key = (tuple(sdims), tuple(sh1[d] for d in sdims), tuple(sh2[d] for d in sdims),
                tuple(input_spacings[0][d] for d in sdims), tuple(input_spacings[1][d] for d in sdims), max_total_pixels_per_stack)
    if memo_key in _BINNING_MEMO:
        return dict(_BINNING_MEMO[memo_key])
    overlap = {d: max(sh1[d], sh2[d]) for d in sdims}
    binning = {d: 1 for d in sdims}
    spacings = input_spacings
    while np.prod([overlap[d] / binning[d] for d in sdims]) >= max_total_pixels_per_stack:
        dim_to_bin = np.argmin([min(spacings[i][d] for i in range(2)) for d in sdims])
        if ndim == 3 and dim_to_bin == 0:
            binning["z"] += 1
        else:
            for d in ["x", "y"]:
                binning[d] += 1
        spacings = [{d: input_spacings[i][d] * binning[d] for d in sdims} for i in range(2)]
    if len(_BINNING_MEMO) > 256:
        _BINNING_MEMO.clear()
    _BINNING_MEMO[memo_key] = dict(binning)
    return binning


_BINNING_MEMO = {}


# =====================================================================================================
# Pair preparation and the register() workflow (host glue around the kernels)
# =====================================================================================================
def _is_axis_aligned(affine, tol=1e-9):
    A = np.asarray(affine)[:-1, :-1]
    return bool(np.all(np.abs(A - np.diag(np.diag(A))) < tol))


def _get_overlap_bboxes(sim1, sim2, input_transform_key=None, output_transform_key=None, overlap_tolerance=None, closed_form=True):
    """registration._get_overlap_bboxes (registration.py:194-277): the two view boxes are intersected as halfspaces in the
    coordinate system of ``input_transform_key`` (mv_graph.py:301-338) and the vertices of the intersection polytope are
    projected into each view's intrinsic frame; lowers / uppers are their extrema.  Axis-aligned pairs (every tile grid)
    take the closed form -- the polytope is the intersection of the world AABBs, whose 2^ndim corners are the vertices;
    rotated / sheared / scaled views go through scipy's linprog + HalfspaceIntersection like the reference.
    Returns None when the views do not overlap."""
    from . import mv_graph
    from . import spatial_image_utils as si_utils
    from .transformation import transform_pts

    sims = [sim1, sim2]
    affines = [param_utils.select_time(si_utils.get_affine_from_sim(s, input_transform_key), 0) for s in sims]
    sps = [si_utils.get_stack_properties_from_sim(s) for s in sims]
    if overlap_tolerance is not None:
        sps = [si_utils_extend(sp, overlap_tolerance) for sp in sps]
    if closed_form and all(_is_axis_aligned(a) for a in affines):
        res = mv_graph.get_overlap_aabb(sps[0], affines[0], sps[1], affines[1])
        if res is None:
            return None
        lo, hi = res
        ndim = len(lo)
        corners = np.array(list(np.ndindex(*([2] * ndim)))) * (hi - lo) + lo
        vol = float(np.prod(hi - lo))
    else:
        # (closed_form=False: the reference's own sequence -- linprog feasible point, Qhull halfspace intersection -- also for
        # axis-aligned pairs, whose vertices then carry Qhull's round-off like the reference's: registration.py:229-239)
        vol, hs = mv_graph.get_overlap_between_pair_of_stack_props(dict(sps[0], transform=affines[0]), dict(sps[1], transform=affines[1]),
                                                                   closed_form=closed_form)
        if hs is None:
            return None
        corners = np.asarray(hs.intersections)
    if output_transform_key is None:
        cts = [transform_pts(corners, np.linalg.inv(a)) for a in affines]
    elif output_transform_key == input_transform_key:
        cts = [corners, corners]
    else:
        raise NotImplementedError
    return {"lowers": [np.min(c, axis=0) for c in cts], "uppers": [np.max(c, axis=0) for c in cts], "vol": float(vol)}


def si_utils_extend(stack_props, extend_by):
    """spatial_image_utils.extend_stack_props (spatial_image_utils.py:889-913) on a copy."""
    sp = {k: dict(v) for k, v in stack_props.items()}
    if not isinstance(extend_by, dict):
        extend_by = {d: extend_by for d in sp["spacing"]}
    for d, val in extend_by.items():
        sp["shape"][d] += int(np.ceil(2 * val / sp["spacing"][d]))
        sp["origin"][d] -= val
    return sp


def _normalise_tolerance(overlap_tolerance, sdims):
    """``overlap_tolerance`` (None, one number, or a dict that may leave dims out) as {dim: float} over ``sdims``."""
    if overlap_tolerance is None:
        return {d: 0.0 for d in sdims}
    if isinstance(overlap_tolerance, (int, float)):
        return {d: float(overlap_tolerance) for d in sdims}
    return {d: float(overlap_tolerance.get(d, 0.0)) for d in sdims}


def _binned_coords(coords, b):
    """Coordinates of an axis binned by ``b`` (``coarsen(boundary="trim").mean()``, registration.py:1732-1741): the mean of
    every group of ``b`` samples -- the sum divided by b, as numpy's mean does it -- a trailing group that is not full dropped.
    ``coords``: one axis (L,) or the same axis of several views stacked (views, L): one reduction for all of them (the same
    additions per element as view by view)."""
    m = coords.shape[-1] // b
    return np.add.reduce(coords[..., : m * b].reshape(coords.shape[:-1] + (m, b)), axis=-1) / b


def _bin_sim(sim, binning, device, wait=True, out=None):
    """sim.coarsen(binning, boundary="trim").mean().astype(dtype) incl. the coarsened coordinates
    (registration.py:1732-1741)."""
    from . import spatial_image_utils as si_utils

    sdims = si_utils.get_spatial_dims_from_sim(sim)
    bins = [int(binning.get(d, 1)) for d in sdims]
    if max(bins) == 1:
        return sim
    if is_device_array(sim.data):
        sim.data.wait_ready(device)      # (an upload still in flight: this lane's stream waits for it)
    data = _reg_ops.bin_mean(sim.data, bins, device, wait=wait) if out is None else _reg_ops.bin_mean(sim.data, bins, device, wait=wait, out=out)
    coords = {d: _binned_coords(np.asarray(sim.coords[d]), b) for d, b in zip(sdims, bins)}
    out = si_utils.SpatialImage(data, sdims, coords, {"transforms": dict(sim.attrs.get("transforms", {}))})
    return out


def sims_to_intrinsic_coord_system(sim1, sim2, transform_key, overlap_bboxes, device=0):
    """registration.sims_to_intrinsic_coord_system (registration.py:280-350): both views resampled (float32,
    NaN outside) onto the fixed view's pixel grid over the overlap box."""
    from . import spatial_image_utils as si_utils
    from .transformation import transform_sim

    sdims = si_utils.get_spatial_dims_from_sim(sim1)
    lowers, uppers = overlap_bboxes
    spacing = np.max([si_utils.get_spacing_from_sim(s, asarray=True) for s in [sim1, sim2]], axis=0)
    affines = [param_utils.select_time(s.attrs["transforms"][transform_key], 0) for s in [sim1, sim2]]
    transf_affine = np.matmul(np.linalg.inv(affines[1]), affines[0])
    shape = np.floor(np.array(uppers[0] - lowers[0]) / spacing + 1).astype(np.uint64)
    osp = {
        "origin": {d: float(lowers[0][i]) for i, d in enumerate(sdims)},
        "spacing": {d: float(spacing[i]) for i, d in enumerate(sdims)},
        "shape": {d: int(shape[i]) for i, d in enumerate(sdims)},
    }
    out = []
    for isim, sim in enumerate([sim1, sim2]):
        # allow_noop=False: the reference's no-op shortcut would hand back the input (already float32 there,
        # transformation.py:102-119); resampling on an identical grid yields the same values as float32
        t = transform_sim(sim, [None, transf_affine][isim], output_stack_properties=osp, mode="constant", cval=np.nan,
                          device=device, allow_noop=False)
        si_utils.set_sim_affine(t, si_utils.get_affine_from_sim(sim1, transform_key), transform_key)
        out.append(t)
    return out[0], out[1]


def get_affine_from_intrinsic_affine(data_affine, sim_fixed, sim_moving, transform_key_fixed=None, transform_key_moving=None):
    """registration.get_affine_from_intrinsic_affine (registration.py:1382-1474), including its use of
    ``transform_key_moving`` for the fixed view (:1423-1425)."""
    from . import spatial_image_utils as si_utils

    n = data_affine.shape[0]
    p2w_fixed = np.eye(n) if transform_key_fixed is None else param_utils.select_time(sim_fixed.attrs["transforms"][transform_key_moving], 0)
    p2w_moving = np.eye(n) if transform_key_moving is None else param_utils.select_time(sim_moving.attrs["transforms"][transform_key_moving], 0)

    def d_to_p(sim):
        return np.matmul(
            param_utils.affine_from_translation(si_utils.get_origin_from_sim(sim, asarray=True)),
            np.diag(list(si_utils.get_spacing_from_sim(sim, asarray=True)) + [1]),
        )

    D_to_W_f = np.matmul(p2w_moving, d_to_p(sim_moving))
    D_to_W_c = np.matmul(p2w_fixed, d_to_p(sim_fixed))
    return np.matmul(D_to_W_f, np.matmul(data_affine, np.linalg.inv(D_to_W_c)))


def dispatch_pairwise_reg_func(pairwise_reg_func, fixed_data=None, moving_data=None, skip_constant_check=False, device=0,
                               **pairwise_reg_func_kwargs):
    """registration.dispatch_pairwise_reg_func (registration.py:1477-1544): constant-image guard + call."""
    if pairwise_reg_func is phase_correlation_registration and fixed_data is not None and moving_data is not None \
            and not skip_constant_check:
        return pairwise_reg_func(fixed_data=fixed_data, moving_data=moving_data, device=device, _constant_check=True,
                                 **pairwise_reg_func_kwargs)
    if fixed_data is not None and moving_data is not None and not skip_constant_check:
        for name, im in (("fixed", fixed_data), ("moving", moving_data)):
            _, mn, mx, _ = _reg_ops.rescale_intensity(_as_array(im), device, out_on_device=is_device_array(_as_array(im)))
            if mn == mx:
                warnings.warn(
                    "An overlap region between tiles/views is all zero or constant. Assuming identity transform.",
                    UserWarning, stacklevel=2,
                )
                nd = _as_array(fixed_data).ndim
                return {"affine_matrix": param_utils.identity_transform(nd), "quality": np.nan}
    if fixed_data is not None:
        pairwise_reg_func_kwargs["fixed_data"] = fixed_data
        pairwise_reg_func_kwargs["moving_data"] = moving_data
    try:
        return pairwise_reg_func(device=device, **pairwise_reg_func_kwargs)
    except TypeError as e:
        if "device" not in str(e):
            raise
        return pairwise_reg_func(**pairwise_reg_func_kwargs)


# ---- lean per-pair host path ----------------------------------------------------------------------------------------
# The generic functions above spend ~0.45 ms of interpreter time per pair in small numpy calls, and every worker thread
# needs the GIL for them: on the north-star mosaic that serial share (144 x 0.45 ms) is a third of the registration time
# (adding 0.3 ms of Python per pair adds 40 ms per step).  For the common case -- views whose transform is a pure
# translation, the built-in phase correlation -- the same steps are done here with plain Python floats, in the same
# order of IEEE operations as the numpy expressions they replace (equality with the generic path is tested on the CPU
# for the plan and on the GPU for the result).
class _TileGeom:
    """What the pair plans need of one (binned) view: its coordinate arrays as lists, origin / spacing / shape as the
    spatial_image_utils getters derive them, and the translation of its transform."""

    __slots__ = ("sim", "sdims", "coords", "origin", "spacing", "shape", "t", "affine", "_src")

    def __init__(self, sim, transform_key, like=None, coords=None):
        self.sim = sim
        dims = sim.dims
        self.sdims = sd = [d for d in ("z", "y", "x") if d in dims]
        # (float64 arrays, not lists: 128 geometries of a 64-tile mosaic were 150 000 float objects to build under the GIL and
        # 2.5 ms to tear down when register() returns; float64 scalars subtract exactly like Python floats)
        co = sim.coords
        # ``coords``: the geometry of a binned version of ``sim`` whose voxels do not exist (the batched pair path plans on it)
        self.coords = cs = coords if coords is not None else [np.ascontiguousarray(co[d], dtype=np.float64) for d in sd]
        self.origin = [float(c[0]) for c in cs]
        self.spacing = [float(c[1] - c[0]) if len(c) > 1 else 1.0 for c in cs]
        self.shape = [len(c) for c in cs]
        src = sim.attrs["transforms"][transform_key]
        self._src = src
        if like is not None and like._src is src:       # the binned view of ``like``'s image: the very same transform array
            self.t, self.affine = like.t, like.affine
            return
        a = param_utils.select_time(np.asarray(src, dtype=np.float64), 0)
        n = len(sd)
        pure = False
        if a.shape == (n + 1, n + 1):
            b = a.copy()
            b[:n, n] = 0.0
            pure = b.tobytes() == _eye_bytes(n)      # (a -0.0 entry counts as "not pure": the generic path handles it)
        self.t = [float(v) for v in a[:n, n]] if pure else None
        self.affine = a


_EYE_BYTES = {}


def _eye_bytes(n):
    if n not in _EYE_BYTES:
        _EYE_BYTES[n] = np.eye(n + 1).tobytes()
    return _EYE_BYTES[n]


def _lean_world_box(g, tol):
    """world_aabb of stack props extended by ``tol`` (si_utils_extend) under a pure translation: per axis
    (fl(o + t), fl(fl(fl((n - 1) s) + o) + t)) with o, n the extended origin / shape."""
    lo, hi = [], []
    for k in range(len(g.sdims)):
        n, o, s = g.shape[k], g.origin[k], g.spacing[k]
        if tol is not None:
            n = n + int(np.ceil(2 * tol[k] / s))
            o = o - tol[k]
        lo.append(o + g.t[k])
        hi.append(((n - 1) * 1.0 * s + o) + g.t[k])
    return lo, hi


def _lean_overlap(g1, g2, tol, to_intrinsic):
    """_get_overlap_bboxes for two translated views: (lowers, uppers) per view, in each view's own frame
    (``to_intrinsic``) or in world coordinates."""
    lo1, hi1 = _lean_world_box(g1, tol)
    lo2, hi2 = _lean_world_box(g2, tol)
    lo = [max(a, b) for a, b in zip(lo1, lo2)]
    hi = [min(a, b) for a, b in zip(hi1, hi2)]
    if any(h < l for l, h in zip(lo, hi)):
        return None
    up = [1.0 * (h - l) + l for l, h in zip(lo, hi)]            # the far corner as the generic path builds it: gv * (hi - lo) + lo
    if not to_intrinsic:
        return [lo, lo], [up, up]
    lowers = [[l + (-t) for l, t in zip(lo, g.t)] for g in (g1, g2)]
    uppers = [[u + (-t) for u, t in zip(up, g.t)] for g in (g1, g2)]
    return lowers, uppers


# ---- crop length on the knife edge (registration.py:229-239, 314-316; mv_graph.py:301-338) ----------------------------------------
# The reference sizes the overlap crop from the vertices Qhull returns for the intersection of the two view boxes:
# floor((upper - lower) / spacing + 1).  For views on one pixel grid that quotient is an integer up to Qhull's round-off, so the
# reference registers N or N - 1 samples along an axis depending on the SIGN of a 1e-13 term that no closed form predicts (it
# depends on linprog's interior point and Qhull's elimination order).  The closed form registers N.  The default mode therefore
# asks the reference's own sequence ONCE per pair geometry whether it lands on N - 1 somewhere (memo below: a register + fuse loop
# over one mosaic pays the ~3 ms per pair once), and only such pairs leave the fast path for the ``overlap_bbox="reference"`` one.
_HOST_UPLOAD_ASYNC = [os.environ.get("MVS_HOST_STREAM", "1") != "0"]      # register() of plain host tiles: pinned staging + asynchronous uploads
_KNIFE_MEMO = {}
_KNIFE_LOCK = threading.Lock()
_KNIFE_CHECK = [os.environ.get("MVS_KNIFE_CHECK", "1") != "0"]


def set_crop_length_check(enabled):
    """Switch the default crop rule's question to the reference's Qhull sequence on or off for this process (on by default; the
    environment variable MVS_KNIFE_CHECK=0 starts a process with it off).  Off: every pair of views on one pixel grid registers the
    closed form's N samples -- the reference registers N - 1 on some of them (BASELINE config C1's pair), so its translation is
    then not guaranteed -- and a mosaic whose geometry has not been seen before saves ~2 ms of host time per pair.  Returns the
    previous setting."""
    old = _KNIFE_CHECK[0]
    _KNIFE_CHECK[0] = bool(enabled)
    return old


def _reference_crop_shape(g1, g2, tol):
    """Crop shape of the pair (binned views ``g1``, ``g2``: _TileGeom) as the reference derives it, or None without overlap."""
    from . import mv_graph
    from .transformation import transform_pts

    sps = []
    for g in (g1, g2):
        sp = {"origin": dict(zip(g.sdims, g.origin)), "spacing": dict(zip(g.sdims, g.spacing)), "shape": dict(zip(g.sdims, g.shape))}
        if any(tol):
            sp = si_utils_extend(sp, dict(zip(g.sdims, tol)))
        sps.append(dict(sp, transform=g.affine))
    vol, hs = mv_graph.get_overlap_between_pair_of_stack_props(sps[0], sps[1], closed_form=False, need_volume=False)
    if hs is None:
        return None
    c = transform_pts(np.asarray(hs.intersections), np.linalg.inv(g1.affine))
    lo, up = np.min(c, axis=0), np.max(c, axis=0)
    out_spacing = np.maximum(np.asarray(g1.spacing), np.asarray(g2.spacing))
    return np.floor((up - lo) / out_spacing + 1).astype(np.int64)


def _knife_key(g1, g2, tol):
    return (tuple(g1.origin), tuple(g1.spacing), tuple(g1.shape), tuple(g1.t), tuple(g2.origin), tuple(g2.spacing), tuple(g2.shape),
            tuple(g2.t), tuple(tol))


def _reference_crop_differs(g1, g2, tol, closed_form_shape):
    """True when the reference's crop of this pair is not the closed form's (one sample shorter along some axis)."""
    if not _KNIFE_CHECK[0]:
        return False
    key = _knife_key(g1, g2, tol)
    with _KNIFE_LOCK:
        hit = _KNIFE_MEMO.get(key)
    if hit is None:
        ref = _reference_crop_shape(g1, g2, tol)
        hit = bool(ref is not None and not np.array_equal(ref, np.asarray(closed_form_shape, dtype=np.int64)))
        with _KNIFE_LOCK:
            if len(_KNIFE_MEMO) > 65536:
                _KNIFE_MEMO.clear()
            _KNIFE_MEMO[key] = hit
    return hit


def _around10(x):
    """np.around(x, 10) for a Python float: rint(x * 1e10) / 1e10 (round() is half-to-even like rint)."""
    return round(x * 1e10) / 1e10


def _lean_pair_plan(g1, g2, tol):
    """Crop windows, output grid and pixel affines of one pair (steps of register_pair_of_msims /
    sims_to_intrinsic_coord_system / get_pixel_affine for translated views).  None when the views do not overlap."""
    import bisect

    ov = _lean_overlap(g1, g2, tol, True)
    if ov is None:
        return None
    lowers, uppers = ov
    n = len(g1.sdims)
    windows, origins, spacings = [], [], []
    for i, g in enumerate((g1, g2)):
        win, o, sp = [], [], []
        for k in range(n):
            c = g.coords[k]
            start = lowers[i][k] - 1e-6 - g.spacing[k]
            stop = uppers[i][k] + 1e-6 + g.spacing[k]
            # (bisect on the array, not np.searchsorted: a numpy call that drops the GIL makes the 16 pair threads queue for it)
            a, b = bisect.bisect_left(c, start), bisect.bisect_right(c, stop)
            if b <= a:
                return None
            win.append((a, b))
            o.append(float(c[a]))
            sp.append(float(c[a + 1] - c[a]) if b - a > 1 else 1.0)
        windows.append(win)
        origins.append(o)
        spacings.append(sp)
    out_spacing = [max(a, b) for a, b in zip(spacings[0], spacings[1])]
    out_origin = list(lowers[0])
    out_shape = [int(np.floor((uppers[0][k] - lowers[0][k]) / out_spacing[k] + 1)) for k in range(n)]
    t_rel = [a + (-b) for a, b in zip(g1.t, g2.t)]              # inv(A2) @ A1 for translations
    mats, offs = [], []
    for i in range(2):
        tt = [0.0] * n if i == 0 else t_rel
        m, o = [], []
        for k in range(n):
            m.append(_around10((1.0 * out_spacing[k]) / spacings[i][k]))
            v = _around10(((tt[k] + 0.0) - (origins[i][k] - out_origin[k])) / spacings[i][k])
            r = float(round(v))
            o.append(r if abs(v - r) <= 1e-6 else v)
        mats.append(m)
        offs.append(o)
    return {"windows": windows, "out_origin": out_origin, "out_spacing": out_spacing, "out_shape": out_shape,
            "matrix_diag": mats, "offset": offs}


def _lean_register_pair(g1b, g2b, g1, g2, sdims, tol, upsample_factor, transform_key, device):
    """register_pair_of_msims for translated views and the built-in phase correlation, on plans made of floats."""
    from . import spatial_image_utils as si_utils
    from .transformation import resample_array

    plan = _lean_pair_plan(g1b, g2b, tol)
    if plan is None:
        raise ValueError("views do not overlap")
    n = len(sdims)
    slabs = [g.sim.data[tuple(slice(a, b) for a, b in plan["windows"][i])] for i, g in enumerate((g1b, g2b))]
    uf = _default_upsample_factor(n) if upsample_factor is None else upsample_factor
    if all(is_device_array(d) and d.dtype in _lib.DTYPE_CODES for d in slabs):
        # resample both crops + register them: one library call, no crop allocation, no wait in between
        t, quality, status, _ = _reg_ops.register_views(slabs[0], plan["matrix_diag"][0], plan["offset"][0], slabs[1], plan["matrix_diag"][1],
                                                        plan["offset"][1], plan["out_shape"], uf, None, True, device)
    else:
        crops = [resample_array(d, np.diag(plan["matrix_diag"][i]), np.array(plan["offset"][i]), plan["out_shape"], 1, np.nan, device)
                 for i, d in enumerate(slabs)]
        t, quality, status, _ = _reg_ops.register_crops(crops[0], crops[1], uf, None, True, device)
    if status == 2:
        warnings.warn("An overlap region between tiles/views is all zero or constant. Assuming identity transform.", UserWarning, stacklevel=3)
        affine, quality = param_utils.identity_transform(n), np.nan
    elif status == 1:
        raise RuntimeError("phase correlation produced no admissible shift candidate (registration.py:479-480)")
    elif status == 3:
        raise ValueError("All-NaN slice encountered")
    else:
        affine = param_utils.affine_from_translation([float(v) for v in t])
    # physical affine (get_affine_from_intrinsic_affine with both transformed crops on the output grid and carrying view 1's
    # transform): kept in numpy, its matmul / inverse chain is part of the result's rounding
    # origin / spacing as the getters read them back from the crops' coordinate arrays (o + s * arange): c[0] and c[1] - c[0]
    eff_spacing = [((o + sp * 1.0) - (o + sp * 0.0)) if nn > 1 else 1.0 for o, sp, nn in zip(plan["out_origin"], plan["out_spacing"], plan["out_shape"])]
    eff_origin = [o + sp * 0.0 for o, sp in zip(plan["out_origin"], plan["out_spacing"])]
    d_to_p = np.matmul(param_utils.affine_from_translation(np.array(eff_origin)), np.diag(eff_spacing + [1]))
    D = np.matmul(g1b.affine, d_to_p)
    affine_phys = np.matmul(D, np.matmul(affine, np.linalg.inv(D)))
    lo, up = _lean_overlap(g1, g2, tol, False)
    return {"transform": affine_phys, "quality": float(quality) if quality is not None else np.nan,
            "bbox": np.array([lo[0], up[0]])}


_lean_enabled = [True]      # tests switch the lean path off to compare it with the generic one
_PREBIN_GROUP = [8]         # tiles per binning launch / ticket of register()'s pre-binning (the pairs of a group's tiles start after it)
_native_graph = [True]      # tests: register() through mv_graph's generic graph functions instead of mvs_view_graph_prune
_native_resolution = [True]     # tests: register() through param_resolution's generic functions instead of mvs_resolve_translations


_JOB_DTYPE = np.dtype(_lib.mvs_pair_job_t)

_pair_timeline = None         # tests / bench: a list that the batched pair path fills with ((i, j), done ticket) per registered pair
_raw_crops_enabled = [True]  # tests: the batched pair path through binned copies of the tiles instead of binning inside the crop kernel
_BATCH_LANES = [8]          # context lanes / native worker threads of the batched pair path when the caller does not say (n_parallel_pairwise_regs)
_batch_enabled = [True]     # tests: compute_pairwise_registrations through the per-pair worker threads instead of mvs_register_pairs


def _pair_results_from_plan(ts, qualities, statuses, out_origin, out_spacing, out_shape, fixed_affines, lo_world, up_world):
    """The result dicts of _lean_register_pair for all pairs at once: the pixel translation of every pair turned into the
    physical affine (get_affine_from_intrinsic_affine with both crops on the fixed view's overlap grid, registration.py:1382-1474)
    -- the same matmul / inverse chain per pair, on stacked (pairs, n + 1, n + 1) arrays -- and the overlap box in world
    coordinates.  Statuses as mvs_register_crops reports them (2: constant overlap -> identity + warning; 1 / 3 raise)."""
    ne, n = ts.shape
    for k in range(ne):      # errors in pair order, like the futures of the worker pool
        if statuses[k] == 1:
            raise RuntimeError("phase correlation produced no admissible shift candidate (registration.py:479-480)")
        if statuses[k] == 3:
            raise ValueError("All-NaN slice encountered")
    const = statuses == 2
    for _ in range(int(np.count_nonzero(const))):
        warnings.warn("An overlap region between tiles/views is all zero or constant. Assuming identity transform.", UserWarning, stacklevel=4)
    affine = np.zeros((ne, n + 1, n + 1))
    affine[:, np.arange(n + 1), np.arange(n + 1)] = 1.0
    affine[:, :n, n] = np.where(const[:, None], 0.0, ts)
    quality = np.where(const, np.nan, qualities)
    # origin / spacing as the getters read them back from the crops' coordinate arrays (o + s * arange): c[0] and c[1] - c[0]
    eff_spacing = np.where(out_shape > 1, (out_origin + out_spacing * 1.0) - (out_origin + out_spacing * 0.0), 1.0)
    eff_origin = out_origin + out_spacing * 0.0
    shift = np.zeros((ne, n + 1, n + 1))
    shift[:, np.arange(n + 1), np.arange(n + 1)] = 1.0
    shift[:, :n, n] = eff_origin
    scale = np.zeros((ne, n + 1, n + 1))
    scale[:, np.arange(n), np.arange(n)] = eff_spacing
    scale[:, n, n] = 1.0
    d_to_p = np.matmul(shift, scale)
    D = np.matmul(fixed_affines, d_to_p)
    affine_phys = np.matmul(D, np.matmul(affine, np.linalg.inv(D)))
    return [{"transform": affine_phys[k], "quality": float(quality[k]), "bbox": np.array([lo_world[k], up_world[k]])} for k in range(ne)]


# ---- the batched pair path, step by step (_register_pairs_batched below is the driver).  Everything but _run_pair_jobs, and
# the binned copies _crop_sources makes when the crops cannot come from the raw tiles, is host code that runs without a device:
# tests/test_pair_batch.py (plans, results), tests/test_pair_batch_steps.py (the other steps, the driver around a stand-in run) ----
class _PairBatch:
    """What the steps share about one covered call (filled by _batch_coverage): the arguments the steps read, the used views
    (``used``: their indices into ``sims``, sorted) with their geometry in that order, and the pairs as indices into ``used``."""

    __slots__ = ("sims", "edges", "transform_key", "registration_binning", "overlap_tolerance", "device", "used", "sdims", "n", "dtype",
                 "binning", "bins", "do_bin", "tol", "geoms", "geoms_b", "pairs")


def _upload_order(sims, edges):
    """The order in which the pairs run while tiles are still on their way to the device (device.to_device_async uploads them in
    list order): by the later tile of each pair, as indices into ``edges``.  None: as given (nothing in flight, or already so)."""
    if not any(is_device_array(getattr(sims[v], "data", None)) and sims[v].data.ready_ticket for e in edges for v in e):
        return None
    order = sorted(range(len(edges)), key=[max(e) for e in edges].__getitem__)
    return None if order == list(range(len(edges))) else order


def _in_edge_order(part, index, n_edges):
    """``part[k]`` is the result of edge ``index[k]``: the list over all ``n_edges`` edges (None where ``index`` names none)."""
    res = [None] * n_edges
    for k, r in zip(index, part):
        res[k] = r
    return res


def _pair_geometry(sims, transform_key, bins):
    """_TileGeom of every view as it is and as the registration binning ``bins`` leaves it (coordinates only -- _bin_sim's -- without
    touching a voxel).  Views of one shape: one reduction per axis for all of them (host time)."""
    geoms = [_TileGeom(s, transform_key) for s in sims]
    if max(bins) == 1:
        return geoms, geoms
    if all(g.shape == geoms[0].shape for g in geoms):
        stacked = [_binned_coords(np.stack([g.coords[k] for g in geoms]), b) for k, b in enumerate(bins)]
        coords = [[st[i] for st in stacked] for i in range(len(geoms))]
    else:
        coords = [[_binned_coords(g.coords[k], b) for k, b in enumerate(bins)] for g in geoms]
    return geoms, [_TileGeom(s, transform_key, like=g, coords=c) for s, g, c in zip(sims, geoms, coords)]


def _batch_coverage(sims, edges, transform_key, registration_binning, overlap_tolerance, device):
    """The _PairBatch of a call the batched path covers, or None: plain device-resident images (no pyramids, spatial dims only) of
    one supported dtype on ``device`` whose rows are contiguous, transforms that are pure translations, one binning for all pairs
    that leaves at least one sample per axis.  Decided on the host, before any library call."""
    from . import msi_utils
    from . import spatial_image_utils as si_utils

    if not edges or any(msi_utils.is_msim(m) for m in sims):
        return None
    b = _PairBatch()
    b.sims, b.edges, b.transform_key, b.device = sims, edges, transform_key, device
    b.registration_binning, b.overlap_tolerance = registration_binning, overlap_tolerance
    b.used = used = sorted({v for e in edges for v in e})
    first = sims[used[0]]
    b.sdims = sdims = si_utils.get_spatial_dims_from_sim(first)
    b.n = len(sdims)
    b.dtype = first.data.dtype
    for v in used:
        s_ = sims[v]
        if list(s_.dims) != list(sdims) or not is_device_array(s_.data) or s_.data.dtype != b.dtype or s_.data.dtype not in _lib.DTYPE_CODES:
            return None
    if registration_binning is None:
        shape0, sp0 = si_utils.get_shape_from_sim(first), si_utils.get_spacing_from_sim(first)
        if any(si_utils.get_shape_from_sim(sims[v]) != shape0 or si_utils.get_spacing_from_sim(sims[v]) != sp0 for v in used[1:]):
            return None                  # the optimal binning would differ between pairs
        b.binning = get_optimal_registration_binning(sims[edges[0][0]], sims[edges[0][1]])
    else:
        b.binning = dict(registration_binning)
    b.do_bin = max(b.binning.values()) > 1
    b.bins = [int(b.binning.get(d, 1)) for d in sdims]
    tol = _normalise_tolerance(overlap_tolerance, sdims)
    b.tol = [tol[d] for d in sdims]
    if not all((sims[v].data.device & 0xff) == (device & 0xff) and sims[v].data.strides[-1] == 1 for v in used):
        return None
    if any(len(sims[v].coords[d]) // bb < 1 for v in used for d, bb in zip(sdims, b.bins)):
        return None                      # a binned axis without a sample
    b.geoms, b.geoms_b = _pair_geometry([sims[v] for v in used], transform_key, b.bins)
    if any(g.t is None for g in b.geoms):
        return None
    slot = {v: i for i, v in enumerate(used)}
    b.pairs = np.array([[slot[i], slot[j]] for i, j in edges], dtype=np.int32).reshape(len(edges), 2)
    return b


def _as_ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


_PairPlans = collections.namedtuple("_PairPlans", "windows out_origin out_spacing out_shape matrix_diag offset status")


def _plan_pairs(geoms, pairs, tol):
    """The binding of mvs_plan_pairs (host code; the arithmetic of _lean_pair_plan): crop windows (pairs, 2, 3, 2), output grid and
    pixel affines (diagonal and offset, (pairs, 2, 3)) of the ``pairs`` (index pairs into ``geoms``), axes in the first ``n`` slots;
    ``status`` 1: the views do not overlap.  None when the library declines the call."""
    n, nv = len(geoms[0].sdims), len(geoms)
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    ne = len(pr)
    cptr = (C.c_void_p * (nv * n))(*[g.coords[k].__array_interface__["data"][0] for g in geoms for k in range(n)])
    clen = np.array([len(g.coords[k]) for g in geoms for k in range(n)], dtype=np.int64)
    tr = np.array([g.t for g in geoms], dtype=np.float64).reshape(nv, n)
    tolv = np.array(tol, dtype=np.float64)
    p = _PairPlans(np.zeros((ne, 2, 3, 2), dtype=np.int64), np.zeros((ne, 3)), np.zeros((ne, 3)), np.ones((ne, 3), dtype=np.int64),
                   np.zeros((ne, 2, 3)), np.zeros((ne, 2, 3)), np.zeros(ne, dtype=np.int32))
    rc = _lib.load().mvs_plan_pairs(n, nv, cptr, _as_ptr(clen, C.c_int64), _as_ptr(tr, C.c_double), _as_ptr(tolv, C.c_double), ne,
                                    _as_ptr(pr, C.c_int32), _as_ptr(p.windows, C.c_int64), _as_ptr(p.out_origin, C.c_double),
                                    _as_ptr(p.out_spacing, C.c_double), _as_ptr(p.out_shape, C.c_int64), _as_ptr(p.matrix_diag, C.c_double),
                                    _as_ptr(p.offset, C.c_double), _as_ptr(p.status, C.c_int32))
    return None if rc != 0 else p


def _world_boxes(geoms, pairs, tol):
    """_lean_overlap(..., to_intrinsic=False) of all ``pairs`` (index pairs into ``geoms``: the UNBINNED views) at once: the lower
    and upper corner of every overlap box in world coordinates, (pairs, n) each."""
    n = len(geoms[0].sdims)
    pr = np.asarray(pairs).reshape(-1, 2)
    tolv = np.array(tol, dtype=np.float64)
    o = np.array([g.origin for g in geoms], dtype=np.float64).reshape(-1, n)
    sp = np.array([g.spacing for g in geoms], dtype=np.float64).reshape(-1, n)
    shp = np.array([g.shape for g in geoms], dtype=np.int64).reshape(-1, n)
    tw = np.array([g.t for g in geoms], dtype=np.float64).reshape(-1, n)
    shp = shp + np.ceil(2 * tolv / sp).astype(np.int64)
    o = o - tolv
    lo_v = o + tw
    hi_v = ((shp - 1) * 1.0 * sp + o) + tw
    lo = np.maximum(lo_v[pr[:, 0]], lo_v[pr[:, 1]])
    hi = np.minimum(hi_v[pr[:, 0]], hi_v[pr[:, 1]])
    return lo, 1.0 * (hi - lo) + lo


def _crops_from_raw_tiles(dtype, do_bin, plans, n):
    """Binned integer tiles whose crops are whole-pixel translations (every regular mosaic): the crops come straight from the RAW
    tiles, the binning applied inside the crop kernel (job.bin) -- no binned copy of a tile is ever made, a pair reads only the slabs
    its overlap needs."""
    return bool(do_bin and _raw_crops_enabled[0] and dtype in (np.dtype(np.uint8), np.dtype(np.uint16))
                and np.all(plans.matrix_diag[:, :, :n] == 1.0) and np.all(plans.offset[:, :, :n] == np.floor(plans.offset[:, :, :n])))


def _crop_sources(b, plans, cache):
    """Where the crops of the batch come from: ``(arrays, tickets, raw_crops, prebin_lane)`` -- per used view the DeviceArray the
    windows index and the ticket a pair's lane waits for before it reads it; whether these are the raw tiles with the binning left
    to the crop kernel (_crops_from_raw_tiles); the lane the binning was queued on, to be waited for after the pairs (or None).
    Otherwise binned tiles serve, pre-binned in groups with stream tickets (_prebin_views).  Counts the pairs in
    ``cache.raw_crops``.  None: a binned copy is not what the plans assume, the caller takes the per-pair path."""
    import functools

    sims, used, device = b.sims, b.used, b.device
    raw_crops = _crops_from_raw_tiles(b.dtype, b.do_bin, plans, b.n)
    prebin_lane = None
    if raw_crops or not b.do_bin:
        arrays = [sims[v].data for v in used]
        # tiles still on their way to the device (device.to_device_async): a pair's lane waits for the uploads of ITS two tiles
        tickets = [a.ready_ticket for a in arrays]
    else:
        bkey = tuple(sorted(b.binning.items()))
        if all(cache.ticket_of((id(sims[v].data), bkey)) is None and (id(sims[v].data), bkey) not in cache._items for v in used):
            # (queues the binning of all views on the last context lane; None: not a regular mosaic, the views are binned one by one below)
            prebin_lane = _prebin_views([sims[v] for v in used], b.binning, device, cache)
        arrays, tickets = [], []
        for v, g in zip(used, b.geoms_b):
            s_ = sims[v]
            key = (id(s_.data), bkey)
            b_ = cache.get_or_compute(key, functools.partial(_bin_sim, s_, b.binning, device), keep=s_.data)
            tickets.append(cache.ticket_of(key) or 0)
            if (b_.data.device & 0xff) != (device & 0xff) or b_.data.strides[-1] != 1 or [len(b_.coords[d]) for d in b.sdims] != g.shape:
                return None
            arrays.append(b_.data)
    cache.raw_crops = len(b.edges) if raw_crops else 0
    return arrays, tickets, raw_crops, prebin_lane


def _fill_pair_jobs(plans, pairs, n, base, strides, itemsize, dtype_code, tickets, bin_scale=None, timed=False):
    """One mvs_pair_job_t per pair: its two crop windows as mvs_view_t (strided windows into the arrays at ``base``, one pointer,
    one row of ``strides`` (in elements) and one ticket per view; ``pairs`` index them) and the output grid.  ``bin_scale``: the bins
    per axis when the arrays are raw tiles (window indices of the binned grid times the bin; job.bin), None when the windows index
    the arrays as they are.  ``timed``: every pair leaves a timed ticket of its last kernel (flags).  Plain numpy, no library."""
    ne = len(pairs)
    jobs = (_lib.mvs_pair_job_t * ne)()
    ja = np.frombuffer(jobs, dtype=_JOB_DTYPE)
    k0 = 3 - n
    base, tk = np.asarray(base, dtype=np.uint64), np.asarray(tickets, dtype=np.uint64)
    strides = np.asarray(strides, dtype=np.int64).reshape(-1, n)
    scale = np.array([1] * n if bin_scale is None else bin_scale, dtype=np.int64)      # binned index -> index of the source array
    for i, name in enumerate(("fixed", "moving")):
        f = ja[name]
        vi = pairs[:, i]
        a, b = plans.windows[:, i, :n, 0] * scale, plans.windows[:, i, :n, 1] * scale
        st = strides[vi]
        f["data"] = base[vi] + (np.sum(a * st, axis=1) * itemsize).astype(np.uint64)
        f["dtype"] = dtype_code
        f["mem"] = _lib.MVS_MEM_DEVICE
        f["shape"][:, :k0] = 1
        f["shape"][:, k0:] = b - a
        if n == 3:
            f["stride"][:] = st
        else:       # a 2D slab is one z plane
            f["stride"][:, 0] = st[:, 0] * (b - a)[:, 0]
            f["stride"][:, 1:] = st
        f["matrix"][:] = 0.0
        f["matrix"][:, [0, 4, 8]] = 1.0
        f["matrix"][:, [(k0 + k) * 4 for k in range(n)]] = plans.matrix_diag[:, i, :n]
        f["offset"][:] = 0.0
        f["offset"][:, k0:] = plans.offset[:, i, :n]
        ja["wait_ticket"][:, i] = tk[vi]
    ja["out_shape"][:, :k0] = 1
    ja["out_shape"][:, k0:] = plans.out_shape[:, :n]
    if bin_scale is not None:
        ja["bin"][:, :k0] = 1
        ja["bin"][:, k0:] = scale
    if timed:
        ja["flags"][:] = 1
    return jobs


def _run_pair_jobs(jobs, edges, n, upsample_factor, n_lanes, device, prebin_lane=None):
    """mvs_register_pairs on ``n_lanes`` context lanes driven by native threads -- the one step of the batched path that needs the
    GPU: ``(shifts (pairs, n), qualities, statuses)`` as mvs_register_views reports them per pair.  ``prebin_lane``: waited for
    when the pairs are done or have failed.  Fills ``_pair_timeline``."""
    ne = len(jobs)
    t3, q = np.zeros((ne, 3)), np.zeros(ne)
    status, ncand, rcs = np.zeros(ne, dtype=np.int32), np.zeros(ne, dtype=np.int32), np.zeros(ne, dtype=np.int32)
    lib = _lib.init(device & 0xff)
    try:
        rc = lib.mvs_register_pairs(device & 0xff, ne, jobs, n, int(upsample_factor), -1, 1, int(n_lanes), _as_ptr(t3, C.c_double),
                                    _as_ptr(q, C.c_double), _as_ptr(status, C.c_int32), _as_ptr(ncand, C.c_int32), _as_ptr(rcs, C.c_int32))
    finally:
        if prebin_lane is not None:
            _lib.synchronize(prebin_lane)      # (done long ago unless a pair failed: nothing stays queued on the caller's tiles)
    _lib.check(rc, device & 0xff, "mvs_register_pairs")
    if _pair_timeline is not None:
        done = np.frombuffer(jobs, dtype=_JOB_DTYPE)["wait_ticket"]
        _pair_timeline.extend((tuple(edges[e]), int(done[e, 0])) for e in range(ne))
    return t3[:, 3 - n:], q, status


def _register_planned_pairs(b, plans, pairwise_reg_func_kwargs, n_lanes, cache):
    """Crop sources -> jobs -> mvs_register_pairs -> the result dicts of all pairs (None: not covered after all)."""
    src = _crop_sources(b, plans, cache)
    if src is None:
        return None
    arrays, tickets, raw_crops, prebin_lane = src
    n = b.n
    jobs = _fill_pair_jobs(plans, b.pairs, n, [a.ptr for a in arrays], [a.strides for a in arrays], b.dtype.itemsize, _lib.DTYPE_CODES[b.dtype],
                           tickets, b.bins if raw_crops else None, _pair_timeline is not None)
    upsample_factor = (pairwise_reg_func_kwargs or {}).get("upsample_factor")
    uf = _default_upsample_factor(n) if upsample_factor is None else upsample_factor
    ts, q, status = _run_pair_jobs(jobs, b.edges, n, uf, n_lanes, b.device, prebin_lane)
    # ---- overlap boxes in world coordinates (_lean_overlap on the UNBINNED views) and the physical affines ----
    lo, up = _world_boxes(b.geoms, b.pairs, b.tol)
    fixed_aff = np.array([g.affine for g in b.geoms_b], dtype=np.float64)[b.pairs[:, 0]]
    return _pair_results_from_plan(ts, q, status, plans.out_origin[:, :n], plans.out_spacing[:, :n], plans.out_shape[:, :n], fixed_aff, lo, up)


class _KnifeQuestion:
    """The crop-length question of one batch (_knife_question): its memo key; ``odd``: the remembered answer (indices of the pairs
    whose reference crop is one sample shorter) or None while ``thread`` is still finding it out, into ``box``."""

    __slots__ = ("key", "odd", "thread", "box")


def _ask_reference_crops(box, geoms, pairs, tol, shapes):
    """(body of the helper thread) ``box["odd"]``: the pairs whose reference crop differs; ``box["error"]``: what was raised."""
    try:
        box["odd"] = [e for e, (i, j) in enumerate(pairs) if _reference_crop_differs(geoms[i], geoms[j], tol, shapes[e])]
    except BaseException as exc:      # noqa: BLE001 - handed to the caller's thread by _knife_answer
        box["error"] = exc


def _knife_question(geoms_b, pairs, tol, out_shapes):
    """Which pairs have a reference crop that is one sample shorter (see _reference_crop_differs)?  They take the
    overlap_bbox="reference" path one by one; the others stay in the batch.  One memo entry per MOSAIC geometry: a list of pair
    indices, looked up with a few hundred bytes."""
    q = _KnifeQuestion()
    q.key = ("mosaic", len(geoms_b[0].sdims), pairs.tobytes(), np.array(tol, dtype=np.float64).tobytes(),
             np.array([[g.t, g.origin, g.spacing, g.shape] for g in geoms_b], dtype=np.float64).tobytes())
    q.thread = q.box = None
    with _KNIFE_LOCK:
        q.odd = _KNIFE_MEMO.get(q.key)
    if q.odd is None:
        # a geometry seen for the first time: the question costs ~2 ms of scipy per pair on the host (GIL-bound), the pairs
        # themselves ~0.3 ms each on the GPU -- so it is asked on a thread of its own WHILE all pairs are registered with the
        # closed-form crops (mvs_register_pairs releases the interpreter lock), and the pairs it names, if any, are registered
        # again through the reference's sequence afterwards: the result is the reference's crop for every pair either way.
        q.box = {}
        q.thread = threading.Thread(target=_ask_reference_crops, args=(q.box, geoms_b, pairs.tolist(), tol, out_shapes.copy()),
                                    name="mvs-crop-length", daemon=True)
        q.thread.start()
    return q


def _knife_answer(q):
    """(first call of a geometry) wait for the crop-length answers and remember them; the pairs they name."""
    q.thread.join()
    if "error" in q.box:
        raise q.box["error"]
    with _KNIFE_LOCK:
        _KNIFE_MEMO[q.key] = q.box["odd"]
    return q.box["odd"]


def _redo_reference_pairs(b, res, odd, pairwise_reg_func_kwargs, cache, raw_before=None):
    """The pairs ``odd`` of ``res`` registered the reference's way (overlap_bbox="reference"), one by one, and counted in
    ``cache.reference_pairs``.  ``raw_before``: ``cache.raw_crops`` before a batched run that registered them too -- those
    closed-form results are discarded, so they leave that count."""
    cache.reference_pairs = len(odd)
    if raw_before is not None and cache.raw_crops > raw_before:
        cache.raw_crops = max(raw_before, cache.raw_crops - len(odd))
    for e in odd:
        i, j = b.edges[e]
        res[e] = register_pair_of_msims(b.sims[i], b.sims[j], b.transform_key, registration_binning=b.registration_binning,
                                        overlap_tolerance=b.overlap_tolerance, pairwise_reg_func_kwargs=pairwise_reg_func_kwargs,
                                        device=b.device, _bin_cache=cache, overlap_bbox="reference")
    return res


def _register_pairs_batched(sims, edges, transform_key, registration_binning, overlap_tolerance, pairwise_reg_func_kwargs, device,
                            n_lanes, cache, knife_check=True):
    """compute_pairwise_registrations for the common case in two library calls: plain device-resident images of one dtype whose
    transforms are pure translations, one binning for all pairs, the built-in phase correlation.  ``mvs_plan_pairs`` derives the
    crop windows and pixel affines of all pairs (host code), ``mvs_register_pairs`` registers them on ``n_lanes`` context lanes
    driven by native threads; the interpreter only assembles the inputs and turns the pixel shifts into physical affines
    (stacked matmuls).  Returns the list of result dicts, or None when the case is not covered (the caller then takes the
    per-pair path).  Same plans, same kernels, same results as _lean_register_pair (tests/test_pair_batch.py, -m gpu tests)."""
    again = (transform_key, registration_binning, overlap_tolerance, pairwise_reg_func_kwargs, device, n_lanes, cache)
    order = _upload_order(sims, edges)
    if order is not None:
        # uploads in flight: the pairs in the order in which their later tile lands, results back in edge order
        part = _register_pairs_batched(sims, [edges[k] for k in order], *again, knife_check=knife_check)
        return None if part is None else _in_edge_order(part, order, len(edges))
    b = _batch_coverage(sims, edges, transform_key, registration_binning, overlap_tolerance, device)
    if b is None:
        return None
    plans = _plan_pairs(b.geoms_b, b.pairs, b.tol)
    if plans is None:
        return None
    if np.any(plans.status != 0):
        raise ValueError("views do not overlap")
    knife = _knife_question(b.geoms_b, b.pairs, b.tol, plans.out_shape[:, :b.n]) if knife_check and _KNIFE_CHECK[0] else None
    if knife is not None and knife.odd:
        # a geometry seen before, with pairs on the knife edge: the others as a batch of their own, those the reference's way
        keep = sorted(set(range(len(edges))) - set(knife.odd))
        part = _register_pairs_batched(sims, [edges[e] for e in keep], *again, knife_check=False) if keep else []
        if part is None:
            return None
        return _redo_reference_pairs(b, _in_edge_order(part, keep, len(edges)), knife.odd, pairwise_reg_func_kwargs, cache)
    asked = knife is not None and knife.thread is not None
    raw_before = getattr(cache, "raw_crops", None)
    try:
        res = _register_planned_pairs(b, plans, pairwise_reg_func_kwargs, n_lanes, cache)
    except BaseException:
        if asked:
            knife.thread.join()
        raise
    odd = _knife_answer(knife) if asked else []
    if res is None or not odd:
        return res
    return _redo_reference_pairs(b, res, odd, pairwise_reg_func_kwargs, cache, raw_before)


def _geom_of(sim, transform_key, cache):
    """_TileGeom of a view, shared by the pairs of one compute_pairwise_registrations call."""
    if cache is None:
        return _TileGeom(sim, transform_key)
    return cache.get_or_compute(("geom", id(sim), transform_key), lambda: _TileGeom(sim, transform_key), keep=sim)


def _select_registration_level(msim1, msim2, registration_binning, reg_res_level):
    """The three branches of registration.py:1639-1717: which resolution level of the two images is registered and which
    binning is still applied to it.  ``reg_res_level`` alone: that level, no binning; with ``registration_binning``: that
    level, the binning divided by the level's downsampling factors (which must divide it); neither / binning alone: the
    (optimal) binning split into the lowest level that divides it and a remainder.  Plain SpatialImages count as
    images with scale0 only.  Returns (sim1, sim2, remaining_binning)."""
    from . import msi_utils
    from . import spatial_image_utils as si_utils

    ms = [m if msi_utils.is_msim(m) else None for m in (msim1, msim2)]

    def level(i, scale_key):
        m = (msim1, msim2)[i]
        return msi_utils.get_sim_from_msim(m, scale=scale_key) if ms[i] is not None else m

    def scale_keys(i):
        return msi_utils.get_sorted_scale_keys(ms[i]) if ms[i] is not None else ["scale0"]

    sim1_0, sim2_0 = level(0, "scale0"), level(1, "scale0")
    sdims = si_utils.get_spatial_dims_from_sim(sim1_0)
    if reg_res_level is not None:
        scale_key = f"scale{reg_res_level}"
        if scale_key not in scale_keys(0) or scale_key not in scale_keys(1):
            raise ValueError(f"Resolution level {reg_res_level} (scale{reg_res_level}) does not exist in the multiscale image")
        sim1, sim2 = level(0, scale_key), level(1, scale_key)
        if registration_binning is None:
            return sim1, sim2, {d: 1 for d in sdims}
        factors = {d: sim1_0.sizes[d] / sim1.sizes[d] for d in sdims}
        for d in sdims:
            if d in registration_binning and registration_binning[d] % int(round(factors[d])) != 0:
                raise ValueError(
                    f"Resolution level {reg_res_level} has downsampling factor {int(round(factors[d]))} for dimension {d}, which "
                    f"is not a divisor of registration_binning[{d}]={registration_binning[d]}")
        # (like the reference, every spatial dim must be present in registration_binning here: registration.py:1674-1677)
        return sim1, sim2, {d: registration_binning[d] // int(round(factors[d])) for d in sdims}
    if registration_binning is None:
        registration_binning = get_optimal_registration_binning(sim1_0, sim2_0)
    if ms[0] is None or len(scale_keys(0)) == 1:
        # (missing dims count as 1, like get_res_level_from_binning_factors: msi_utils.py:688-773)
        return sim1_0, sim2_0, {d: registration_binning.get(d, 1) for d in sdims}
    scale_key, remaining = msi_utils.get_res_level_from_binning_factors(ms[0], registration_binning)
    if scale_key not in scale_keys(1):
        raise ValueError(f"{scale_key} does not exist in the second multiscale image")
    return level(0, scale_key), level(1, scale_key), remaining


def _has_keyword(func, keyword):
    """misc_utils.has_keyword: does ``func`` accept ``keyword``?"""
    import inspect

    try:
        return keyword in inspect.signature(func).parameters
    except (TypeError, ValueError):
        return False


def _is_point_aware(pairwise_reg_func):
    """registration.py:1814-1839: a function that takes ``fixed_points`` and ``moving_points`` gets the views' point sets; one
    that takes only one of the two is refused."""
    has = [_has_keyword(pairwise_reg_func, k) for k in ("fixed_points", "moving_points")]
    if any(has) and not all(has):
        raise ValueError("Point-aware pairwise registration functions must accept both 'fixed_points' and 'moving_points'.")
    return all(has)


def _points_for_registration(sim, points_key, sdims, affine, window=None):
    """registration.py:568-592, 1862-1887: the view's point set ``points_key`` -- restricted to the closed ``window``
    ({dim: slice}) when there is one -- without rows that hold a non-finite coordinate, mapped by the view's ``affine``."""
    from . import spatial_image_utils as si_utils
    from .transformation import transform_pts

    points = np.asarray(si_utils.get_point_set(sim, points_key), dtype=np.float64)
    if window is not None:
        points = si_utils.point_set_sel_coords(points, sdims, window)
    points = points[np.all(np.isfinite(points), axis=1)]
    return points if points.size == 0 else transform_pts(points, affine)


def _is_plain_phase_correlation(func, kwargs):
    """The built-in phase correlation with at most ``upsample_factor`` set: what the lean and the batched pair paths cover."""
    return func is phase_correlation_registration and set(kwargs or {}) <= {"upsample_factor"}


def _binned_view(sim, binning, device, cache):
    """``sim`` binned by ``binning`` (the image itself when no axis is binned); with a ``cache`` every tile is binned once."""
    if max(binning.values()) <= 1:
        return sim
    if cache is None:
        return _bin_sim(sim, binning, device)
    key = (id(sim.data), tuple(sorted(binning.items())))
    # (the cache slot keeps sim.data alive, so its id() cannot be recycled for another tile while the cache lives)
    out = cache.get_or_compute(key, lambda: _bin_sim(sim, binning, device), keep=sim.data)
    ticket = cache.ticket_of(key)
    if ticket is not None:       # pre-binned on another lane, possibly still in flight: this lane's stream waits for it (no host wait)
        _lib.check(_lib.init(device).mvs_event_wait(device, ticket), device, "mvs_event_wait")
    return out


def _lean_pair_applies(sim1, sim2, sdims, closed_form, pairwise_reg_func, pairwise_reg_func_kwargs):
    """The gate of _lean_register_pair: the default crop rule, the plain phase correlation, views without non-spatial dims."""
    return closed_form and _is_plain_phase_correlation(pairwise_reg_func, pairwise_reg_func_kwargs) and _lean_enabled[0] \
        and all(list(s_.dims) == list(sdims) for s_ in (sim1, sim2))


def _pair_crop_boxes(sims_b, sdims, transform_key, overlap_tolerance, closed_form):
    """The overlap boxes the pair's crops are cut to, and whether they are the closed form's: ``(ov, closed_form)``.  A pair whose
    closed-form crop is not as long as the reference's takes the reference's boxes (the generic path -- user registration functions,
    scaled views: the same rule as the fast paths, see _reference_crop_differs)."""
    ov = _get_overlap_bboxes(sims_b[0], sims_b[1], transform_key, None, overlap_tolerance, closed_form=closed_form)
    if ov is None:
        raise ValueError("views do not overlap")
    if closed_form and _KNIFE_CHECK[0]:
        ov_ref = _get_overlap_bboxes(sims_b[0], sims_b[1], transform_key, None, overlap_tolerance, closed_form=False)
        if ov_ref is not None:
            osp = np.maximum(*[np.array([si_utils.get_spacing_from_sim(s)[d] for d in sdims]) for s in sims_b])
            n_cf = np.floor((ov["uppers"][0] - ov["lowers"][0]) / osp + 1)
            n_ref = np.floor((ov_ref["uppers"][0] - ov_ref["lowers"][0]) / osp + 1)
            if not np.array_equal(n_cf, n_ref):
                return ov_ref, False
    return ov, closed_form


def _crop_windows(sims_b, sdims, ov, tol=1e-6):
    """Per view the coordinate selection {dim: slice} of its crop: its overlap box widened by one sample and ``tol`` on either side."""
    spacings = [si_utils.get_spacing_from_sim(s) for s in sims_b]
    return [{d: slice(ov["lowers"][i][k] - tol - spacings[i][d], ov["uppers"][i][k] + tol + spacings[i][d]) for k, d in enumerate(sdims)}
            for i in range(2)]


def _register_pair_points(sims, sims_b, sdims, windows, transform_key, points_key, prefilter_markers, pairwise_reg_func,
                          pairwise_reg_func_kwargs, device):
    """The point branch (registration.py:1839-1924): the function works in the space of transform_key.  Returns (transform, quality)."""
    affines = [param_utils.select_time(si_utils.get_affine_from_sim(s_, transform_key), 0) for s_ in sims]
    kw = dict(pairwise_reg_func_kwargs)
    for name, s_, a_, w_ in zip(("fixed", "moving"), sims, affines, windows):
        kw[f"{name}_points"] = _points_for_registration(s_, points_key, sdims, a_, w_ if prefilter_markers else None)
    takes_data = [_has_keyword(pairwise_reg_func, k) for k in ("fixed_data", "moving_data")]
    if any(takes_data) and not all(takes_data):
        raise ValueError("Image-aware pairwise registration functions must accept both 'fixed_data' and 'moving_data'.")
    crops = [si_utils.sim_sel_coords(s_, w_) for s_, w_ in zip(sims_b, windows)] if all(takes_data) or any(
        _has_keyword(pairwise_reg_func, f"{n}_{q}") for n in ("fixed", "moving") for q in ("origin", "spacing")) else None
    for name, k in (("fixed", 0), ("moving", 1)):
        if _has_keyword(pairwise_reg_func, f"{name}_origin"):
            kw[f"{name}_origin"] = si_utils.get_origin_from_sim(crops[k])
        if _has_keyword(pairwise_reg_func, f"{name}_spacing"):
            kw[f"{name}_spacing"] = si_utils.get_spacing_from_sim(crops[k])
    if _has_keyword(pairwise_reg_func, "initial_affine"):
        kw["initial_affine"] = np.matmul(np.linalg.inv(affines[1]), affines[0])
    res = dispatch_pairwise_reg_func(pairwise_reg_func, fixed_data=crops[0].data if all(takes_data) else None,
                                     moving_data=crops[1].data if all(takes_data) else None, skip_constant_check=True, device=device, **kw)
    return np.asarray(res["affine_matrix"], dtype=np.float64), res["quality"]


def _register_pair_pixels(sims_b, windows, ov, transform_key, pairwise_reg_func, pairwise_reg_func_kwargs, device):
    """The pixel branch: both crops resampled onto the fixed view's grid, the function's pixel affine made physical.  Returns
    (transform, quality)."""
    crops = [si_utils.sim_sel_coords(sim, windows[i]) for i, sim in enumerate(sims_b)]
    fixed, moving = sims_to_intrinsic_coord_system(crops[0], crops[1], transform_key, (ov["lowers"], ov["uppers"]), device)
    res = dispatch_pairwise_reg_func(pairwise_reg_func, fixed_data=fixed, moving_data=moving, device=device,
                                     **pairwise_reg_func_kwargs)
    if isinstance(res, list):   # Q2: the reference's `[zeros(ndim)]` return is unusable downstream; surface it
        raise RuntimeError("phase correlation produced no admissible shift candidate (registration.py:479-480)")
    affine = np.asarray(res["affine_matrix"], dtype=np.float64)
    return get_affine_from_intrinsic_affine(affine, fixed, moving, transform_key, transform_key), res["quality"]


def _pair_result(transform, quality, sim1, sim2, transform_key, overlap_tolerance, closed_form):
    """The result of a registered pair: its physical transform, its quality (None: NaN) and the pair's overlap box in world space."""
    ovp = _get_overlap_bboxes(sim1, sim2, transform_key, transform_key, overlap_tolerance, closed_form=closed_form)
    return {"transform": transform, "quality": float(quality) if quality is not None else np.nan,
            "bbox": np.array([ovp["lowers"][0], ovp["uppers"][0]])}


def register_pair_of_msims(msim1, msim2, transform_key, registration_binning=None, overlap_tolerance=None,
                           pairwise_reg_func=phase_correlation_registration, pairwise_reg_func_kwargs=None, device=0,
                           _bin_cache=None, reg_res_level=None, overlap_bbox="closed_form", points_key="beads", prefilter_markers=False):
    """registration.register_pair_of_msims (registration.py:1547-2058) for pixel-space registration functions
    (the form the reference's phase correlation has): returns {"transform", "quality", "bbox"}.  ``reg_res_level`` /
    ``registration_binning`` pick the pyramid level of multiscale inputs as the reference does (registration.py:1639-1717).

    A ``pairwise_reg_func`` that accepts ``fixed_points`` and ``moving_points`` (``registration_marker_based``) takes the
    reference's point branch instead (registration.py:1839-1924, 2029-2030): it is called with the point sets ``points_key`` of
    the two views, each mapped by its view's affine at ``transform_key``, and what it returns is the physical transform.
    ``prefilter_markers`` first restricts every view's points to its overlap window (the closed interval of the crop
    selection: lower - 1e-6 - spacing ... upper + 1e-6 + spacing per dim, in the view's own frame).  Image crops are passed
    only to a function that also takes ``fixed_data`` / ``moving_data``."""
    pairwise_reg_func_kwargs = dict(pairwise_reg_func_kwargs or {})
    point_aware = _is_point_aware(pairwise_reg_func)
    sim1, sim2, registration_binning = _select_registration_level(msim1, msim2, registration_binning, reg_res_level)
    for s_ in (sim1, sim2):
        if is_device_array(s_.data):
            s_.data.wait_ready(device)       # (tiles uploaded with device.to_device_async: this lane's stream waits for them)
    sdims = si_utils.get_spatial_dims_from_sim(sim1)
    overlap_tolerance = _normalise_tolerance(overlap_tolerance, sdims)
    if overlap_bbox not in ("closed_form", "reference"):
        raise ValueError("overlap_bbox must be 'closed_form' or 'reference'")
    closed_form = overlap_bbox == "closed_form"
    sims_b = [_binned_view(s_, registration_binning, device, _bin_cache) for s_ in (sim1, sim2)]
    if _lean_pair_applies(sim1, sim2, sdims, closed_form, pairwise_reg_func, pairwise_reg_func_kwargs):
        geoms = [_geom_of(s_, transform_key, _bin_cache) for s_ in (sims_b[0], sims_b[1], sim1, sim2)]
        if all(g.t is not None for g in geoms):
            tol_l = [overlap_tolerance[d] for d in sdims]
            plan = _lean_pair_plan(geoms[0], geoms[1], tol_l) if _KNIFE_CHECK[0] else None
            if plan is None or not _reference_crop_differs(geoms[0], geoms[1], tol_l, plan["out_shape"]):
                return _lean_register_pair(geoms[0], geoms[1], geoms[2], geoms[3], sdims, tol_l,
                                           pairwise_reg_func_kwargs.get("upsample_factor"), transform_key, device)
            closed_form = False      # the reference registers a crop one sample shorter: this pair takes its sequence
    ov, closed_form = _pair_crop_boxes(sims_b, sdims, transform_key, overlap_tolerance, closed_form)
    windows = _crop_windows(sims_b, sdims, ov)
    if point_aware:
        transform, quality = _register_pair_points((sim1, sim2), sims_b, sdims, windows, transform_key, points_key, prefilter_markers,
                                                   pairwise_reg_func, pairwise_reg_func_kwargs, device)
    else:
        transform, quality = _register_pair_pixels(sims_b, windows, ov, transform_key, pairwise_reg_func, pairwise_reg_func_kwargs, device)
    return _pair_result(transform, quality, sim1, sim2, transform_key, overlap_tolerance, closed_form)


def _prebin_views(sims, registration_binning, device, cache):
    """Queues the binning of all views of a regular mosaic (one shape, one spacing: every pair asks for the same binning)
    on the last context lane and puts the results into ``cache``; returns that lane's device id (to be synchronised before
    the pairs have run) or None when there is nothing to do.  The batched pair path calls this when the crops cannot come from
    the raw tiles (_crop_sources): the tiles are binned in groups, and a pair starts when the groups of its two tiles are done.
    (A helper thread doing the same through the blocking call starves on the GIL: measured.)"""
    from . import spatial_image_utils as si_utils
    from .device import is_device_array

    if len(sims) < 2 or any("t" in s.dims or "c" in s.dims or not is_device_array(s.data) for s in sims):
        return None
    shape0, sp0 = si_utils.get_shape_from_sim(sims[0]), si_utils.get_spacing_from_sim(sims[0])
    for s in sims[1:]:
        if si_utils.get_shape_from_sim(s) != shape0 or si_utils.get_spacing_from_sim(s) != sp0:
            return None
    binning = registration_binning if registration_binning is not None else get_optimal_registration_binning(sims[0], sims[1])
    if max(binning.values()) <= 1:
        return None
    bkey = tuple(sorted(binning.items()))
    lane_device = (device & 0xff) | (15 << 8)        # the last context lane: the pair workers take lanes from 0 upwards

    import ctypes as C

    from .device import DeviceArray
    from .transformation import shape3

    sdims = si_utils.get_spatial_dims_from_sim(sims[0])
    bins = [int(binning.get(d, 1)) for d in sdims]
    dtype = np.dtype(sims[0].data.dtype)
    if dtype not in _lib.DTYPE_CODES or any(tuple(s.data.shape) != tuple(sims[0].data.shape) or s.data.dtype != dtype for s in sims):
        return None
    nd = len(sdims)
    shape = [int(v) for v in sims[0].data.shape]
    oshape = tuple(n // b for n, b in zip(shape, bins))
    datas = [s.data.on_device(lane_device).wait_ready(lane_device) for s in sims]      # (uploads in flight: the binning lane waits for them)
    st0 = tuple(datas[0].strides)
    if any(tuple(d.strides) != st0 for d in datas):
        return None
    pool = DeviceArray.empty((len(sims),) + oshape, dtype, lane_device)     # one allocation for all binned tiles
    lib = _lib.init(lane_device)
    st = [int(v) for v in st0]
    st3 = st if nd == 3 else [st[0] * shape[0], st[0], st[1]]
    s3, b3, st3 = _lib.i64x3(shape3(shape)), _lib.i64x3([1] * (3 - nd) + bins), _lib.i64x3(st3)
    code = _lib.DTYPE_CODES[dtype]
    # the coarsened coordinates of _bin_sim, all views of an axis in one reduction
    all_coords = {d: _binned_coords(np.stack([np.asarray(s.coords[d]) for s in sims]), b) for d, b in zip(sdims, bins)}
    # the tiles are binned in groups (one library call and one ticket each): a pair starts as soon as the groups of its two
    # tiles are done, while the later groups are still being binned (mvs_event_record / mvs_event_wait, no host wait)
    n_v = len(sims)
    item = int(np.prod(oshape)) * dtype.itemsize
    group = max(1, _PREBIN_GROUP[0])
    tickets = []
    for g0 in range(0, n_v, group):
        g1 = min(g0 + group, n_v)
        ins = (C.c_void_p * (g1 - g0))(*[datas[i].ptr for i in range(g0, g1)])
        outs = (C.c_void_p * (g1 - g0))(*[pool.ptr + i * item for i in range(g0, g1)])
        _lib.check(lib.mvs_bin_mean_batch_async(lane_device, g1 - g0, ins, code, s3, st3, b3, outs), lane_device, "mvs_bin_mean_batch_async")
        tk = C.c_uint64(0)
        _lib.check(lib.mvs_event_record(lane_device, C.byref(tk)), lane_device, "mvs_event_record")
        tickets.append(int(tk.value))
    tdims = tuple(sdims)
    ostr = tuple(int(np.prod(oshape[i + 1:])) for i in range(nd))
    for i, s in enumerate(sims):
        out = DeviceArray(pool._buf, pool.ptr + i * item, oshape, ostr, dtype, lane_device)
        coords = {d: all_coords[d][i] for d in sdims}
        # (coordinates of the right lengths by construction: no checks)
        binned = si_utils.SpatialImage._from_parts(out, tdims, coords, {"transforms": dict(s.attrs.get("transforms", {}))}, None)
        cache.put((id(s.data), bkey), binned, keep=(s.data, datas[i]), ticket=tickets[i // group])
    return lane_device


def compute_pairwise_registrations(msims, edges, transform_key, registration_binning=None, overlap_tolerance=0.0,
                                   pairwise_reg_func=phase_correlation_registration, pairwise_reg_func_kwargs=None,
                                   pairwise_executor=None, device=0, host_threads=None, _bin_cache=None, reg_res_level=None,
                                   overlap_bbox="closed_form", points_key="beads", prefilter_markers=False):
    """registration.compute_pairwise_registrations (registration.py:2622-2714): either hand all edges to a
    user ``pairwise_executor(msims, edges, register_kwargs)`` or loop over them on one device.  ``points_key`` /
    ``prefilter_markers`` go to ``register_pair_of_msims`` (point-aware registration functions)."""
    register_kwargs = _executor_kwargs(transform_key, registration_binning, overlap_tolerance, pairwise_reg_func, pairwise_reg_func_kwargs,
                                       reg_res_level, overlap_bbox, points_key, prefilter_markers)
    if pairwise_executor is not None:
        results = pairwise_executor(msims, list(edges), register_kwargs)
        if len(results) != len(edges):
            raise ValueError("pairwise_executor must return one result per edge")
        return results
    cache = _bin_cache if _bin_cache is not None else _BinCache()
    edges = list(edges)
    n_threads = max(1, min(16 if host_threads is None else int(host_threads), len(edges), 16))   # 16 = context lanes per GPU (MVS_MAX_LANES)
    if _batched_route_applies(pairwise_reg_func, pairwise_reg_func_kwargs, reg_res_level, overlap_bbox):
        # all pairs in two library calls (plans + registrations on native worker threads): no interpreter in the pair loop
        # (native workers spin inside the HIP runtime between launches: 6-12 of them reach the GPU's pair throughput, 16 exhaust a
        # 16-core CPU quota and are throttled to half speed -- profiles/round5_lanes.txt; the default is 8)
        batched = _register_pairs_batched(msims, edges, transform_key, registration_binning, overlap_tolerance, pairwise_reg_func_kwargs,
                                          device, min(n_threads, _BATCH_LANES[0] if host_threads is None else 12), cache)
        if batched is not None:
            return batched
    if n_threads == 1:
        return [register_pair_of_msims(msims[i], msims[j], device=device, _bin_cache=cache, **register_kwargs) for i, j in edges]
    # Pairs are independent.  Every call into libmvs_hip.so releases the GIL; each worker thread drives its own
    # context lane (stream + scratch + lock) of the GPU, so the kernels of one pair fill the host round trips and
    # the Python glue of another.  Results keep the order of `edges`.
    pool, lanes, lane_lock = _pair_pool(n_threads)
    futs = [pool.submit(_register_pair_on_own_lane, lanes, lane_lock, msims[i], msims[j], device, cache, register_kwargs) for i, j in edges]
    return [f.result() for f in futs]


def _executor_kwargs(transform_key, registration_binning, overlap_tolerance, pairwise_reg_func, pairwise_reg_func_kwargs, reg_res_level,
                     overlap_bbox, points_key, prefilter_markers):
    """The keywords of register_pair_of_msims that a pairwise executor (and the per-pair loop) is handed.  The last four are
    absent unless set: executors written for the first five keep working."""
    register_kwargs = dict(transform_key=transform_key, registration_binning=registration_binning,
                           overlap_tolerance=overlap_tolerance, pairwise_reg_func=pairwise_reg_func,
                           pairwise_reg_func_kwargs=pairwise_reg_func_kwargs)
    if reg_res_level is not None:
        register_kwargs["reg_res_level"] = reg_res_level
    if overlap_bbox != "closed_form":
        register_kwargs["overlap_bbox"] = overlap_bbox
    if points_key != "beads":
        register_kwargs["points_key"] = points_key
    if prefilter_markers:
        register_kwargs["prefilter_markers"] = True
    return register_kwargs


def _batched_route_applies(pairwise_reg_func, pairwise_reg_func_kwargs, reg_res_level, overlap_bbox):
    """The gate of _register_pairs_batched (which may still decline: _batch_coverage looks at the views)."""
    return _batch_enabled[0] and _lean_enabled[0] and overlap_bbox == "closed_form" \
        and _is_plain_phase_correlation(pairwise_reg_func, pairwise_reg_func_kwargs) and reg_res_level is None


def _register_pair_on_own_lane(lanes, lane_lock, msim1, msim2, device, cache, register_kwargs):
    """A pair on a worker thread of _pair_pool: each thread owns one context lane of the GPU (`device | lane << 8`: own stream,
    scratch and lock)."""
    tid = threading.get_ident()
    with lane_lock:
        lane = lanes.setdefault(tid, len(lanes))
    return register_pair_of_msims(msim1, msim2, device=(device & 0xff) | (lane << 8), _bin_cache=cache, **register_kwargs)


_PAIR_POOLS = {}
_PAIR_POOLS_LOCK = threading.Lock()


def _pair_pool(n_threads):
    """The worker threads of compute_pairwise_registrations live across calls (starting 16 threads costs ~10 ms of the
    first pairs' time in every call otherwise); one pool per thread count, with its thread -> lane table."""
    from concurrent.futures import ThreadPoolExecutor

    with _PAIR_POOLS_LOCK:
        entry = _PAIR_POOLS.get(n_threads)
        if entry is None:
            from .executors import pin_worker_thread

            # the workers keep to one compact block of CPUs (see executors.pin_process_to_compact_cpus: spread over both sockets
            # of a large host they lose ~10 % of the pairwise wall); the caller's own threads are not touched
            entry = _PAIR_POOLS[n_threads] = (ThreadPoolExecutor(max_workers=n_threads, thread_name_prefix="mvs-pair",
                                                                 initializer=pin_worker_thread), {}, threading.Lock())
        return entry


def _set_event():
    import threading

    e = threading.Event()
    e.set()
    return e


_FINISHED = _set_event()


class _BinCache:
    """Binned tiles shared by the pairs of one compute_pairwise_registrations call (each tile is binned once).
    Thread safe: the first thread asking for a key computes it, the others wait for that result."""

    def __init__(self):
        import threading

        self._lock = threading.Lock()
        self._items = {}
        self.hits = self.misses = 0      # (tests: the pre-binned tiles of register() must be found by every pair)
        self.raw_crops = 0               # pairs whose crops were taken from the raw tiles (no binned copies at all)
        self.reference_pairs = 0         # pairs the default crop rule sent through the reference's Qhull sequence (N - 1 samples)

    def put(self, key, value, keep=None, ticket=None):
        """Store a finished value (``keep``: the objects whose id() is part of ``key``; the slot holds them alive).  ``ticket``:
        the value's device memory is complete once this mvs_event_record ticket has passed -- a lane that reads it first makes
        its stream wait for the ticket (``ticket_of``)."""
        slot = {"event": _FINISHED, "value": value, "error": None, "keep": keep, "ticket": ticket}      # (one shared, already set event)
        with self._lock:
            self._items[key] = slot

    def ticket_of(self, key):
        slot = self._items.get(key)
        return None if slot is None else slot.get("ticket")

    def get_or_compute(self, key, fn, keep=None):
        """``keep``: the object whose id() is part of ``key``; the slot holds a reference to it."""
        import threading

        with self._lock:
            slot = self._items.get(key)
            owner = slot is None
            if key[0] != "geom":          # (the statistics count the binned tiles)
                if owner:
                    self.misses += 1
                else:
                    self.hits += 1
            if owner:
                slot = self._items[key] = {"event": threading.Event(), "value": None, "error": None, "keep": keep}
        if owner:
            try:
                slot["value"] = fn()
            except BaseException as e:   # noqa: BLE001 - re-raised in every waiter
                slot["error"] = e
            slot["event"].set()
        else:
            slot["event"].wait()
        if slot["error"] is not None:
            raise slot["error"]
        return slot["value"]


def resolve_translations(n_views, edges, pair_results, reference_view=0, weights=None):
    """Minimal groupwise resolution for translation-only pairwise results: least squares on
    tau_j - tau_i = -d_ij with tau_ref = 0 (each connected component gets its own reference).

    Not the reference's method (that is ``param_resolution.groupwise_resolution``); kept as
    ``groupwise_resolution_method="linear"``: the fixed point of the reference's bead sweeps on a translation graph
    when no edge is pruned, in one solve."""
    ndim = np.asarray(pair_results[0]["transform"]).shape[0] - 1 if pair_results else 0
    params = [np.eye(ndim + 1) for _ in range(n_views)]
    if not edges:
        return params
    adj = {v: set() for v in range(n_views)}
    for i, j in edges:
        adj[i].add(j)
        adj[j].add(i)
    seen = set()
    for start in range(n_views):
        if start in seen:
            continue
        comp, stack = [], [start]
        seen.add(start)
        while stack:
            v = stack.pop()
            comp.append(v)
            for w in adj[v]:
                if w not in seen:
                    seen.add(w)
                    stack.append(w)
        comp = sorted(comp)
        if len(comp) == 1:
            continue
        ref = reference_view if reference_view in comp else comp[0]
        idx = {v: k for k, v in enumerate(comp)}
        rows, rhs, wts = [], [], []
        for k, (i, j) in enumerate(edges):
            if i not in idx:
                continue
            r = np.zeros(len(comp))
            r[idx[j]] = 1.0
            r[idx[i]] = -1.0
            rows.append(r)
            rhs.append(-np.asarray(pair_results[k]["transform"])[:ndim, ndim])
            wts.append(1.0 if weights is None else float(weights[k]))
        A = np.array(rows) * np.sqrt(np.array(wts))[:, None]
        B = np.array(rhs) * np.sqrt(np.array(wts))[:, None]
        anchor = np.zeros((1, len(comp)))
        anchor[0, idx[ref]] = 1e3
        A = np.vstack([A, anchor])
        B = np.vstack([B, np.zeros((1, ndim))])
        tau, *_ = np.linalg.lstsq(A, B, rcond=None)
        tau -= tau[idx[ref]]
        for v in comp:
            params[v] = param_utils.affine_from_translation(tau[idx[v]])
    return params


class _RegisterCall:
    """The state of one ``register`` call; every step below reads and fills it.  The arguments of ``register()`` under their own
    names, and:

    sims              the views as plain SpatialImages (scale0 of a multiscale image), all channels
    ci                index of the registration channel (0 when there is no choice to make)
    sims_reg          ``sims`` reduced to that channel: what is registered (device-resident copies once the upload is staged)
    nt                number of time points
    multiscale        pyramid levels take part: an image has more than scale0 or ``reg_res_level`` is given (set before the upload
                      gate, which asks for it; the levels themselves are only built when it holds, and then nothing is uploaded)
    levels_reg        per view the registration channel of every pyramid level, scale0 first (only when ``multiscale``)
    bin_cache         the binned tiles the pairs of the call share (None with an executor, time points or pyramid levels)
    sps, affs         per view: the stack properties, the affine under ``transform_key`` at time point 0
    edges             the pairs that get registered, sorted ``(i, j)`` with ``i < j``
    params_t          per time point the resolved parameters, one matrix per view
    all_results       per time point the pair results, in the order of ``edges``
    resolution_info   per time point what the groupwise resolution reports (None for "linear")
    """

    def __init__(self, **arguments):
        self.__dict__.update(arguments)
        self.params_t, self.all_results, self.resolution_info = [], [], []


def _channel_of(s, ci):
    return s.isel({"c": ci}) if "c" in s.dims else s


def _registration_channel(call):
    """``sims``, ``ci``, ``sims_reg``, ``nt``: the plain images, the channel that is registered, and the time points."""
    call.sims = sims = [msi_utils.get_sim_from_msim(m) if msi_utils.is_msim(m) else m for m in call.msims]
    call.ci = 0
    if "c" in sims[0].dims and sims[0].sizes["c"] > 1:
        if call.reg_channel is None and call.reg_channel_index is None:
            raise Exception("Please choose a registration channel.")
        call.ci = call.reg_channel_index if call.reg_channel is None else int(np.nonzero(sims[0].coords["c"] == call.reg_channel)[0][0])
    call.sims_reg = [_channel_of(s, call.ci) for s in sims]
    call.nt = call.sims_reg[0].sizes.get("t", 1) if "t" in call.sims_reg[0].dims else 1


def _pyramid_levels(call):
    """``multiscale``, ``levels_reg``, ``bin_cache``.  Pyramid levels take part only when an image has more than scale0 or a level
    is asked for (registration.py:1639-1717)."""
    call.multiscale = call.reg_res_level is not None or any(msi_utils.is_msim(m) and len(m.keys()) > 1 for m in call.msims)
    call.levels_reg = [[_channel_of(msi_utils.get_sim_from_msim(m, scale=k), call.ci) for k in msi_utils.get_sorted_scale_keys(m)]
                       if msi_utils.is_msim(m) else [_channel_of(m, call.ci)] for m in call.msims] if call.multiscale else None
    # (binned copies of the tiles are only made when the batched pair path cannot take its crops from the raw tiles: it then
    # queues the binning of all views itself, in groups with stream tickets -- see _crop_sources / _prebin_views)
    call.bin_cache = _BinCache() if call.pairwise_executor is None and call.nt == 1 and not call.multiscale else None


def _wants_async_upload(call):
    """Plain host numpy tiles (or windows of Zarr arrays) of 256 MiB and more -- what a user of the reference hands over -- for the
    built-in pair path on scale0.  (Whatever ``pairwise_reg_func_kwargs`` holds: the upload serves the per-pair paths as well as
    the batched one, so the function alone is asked about.)"""
    sims_reg = call.sims_reg
    return _HOST_UPLOAD_ASYNC[0] and call.pairwise_executor is None and not call.multiscale \
        and _is_plain_phase_correlation(call.pairwise_reg_func, None) \
        and all((isinstance(s.data, np.ndarray) or type(s.data).__name__ in ("ZarrArray", "ZarrView"))
                and list(s.dims) == list(si_utils.get_spatial_dims_from_sim(s)) for s in sims_reg) \
        and sum(int(np.prod(s.data.shape)) * np.dtype(s.data.dtype).itemsize for s in sims_reg) >= (256 << 20) and _lib.device_count() > 0 \
        and all(np.dtype(s.data.dtype) in _lib.DTYPE_CODES for s in sims_reg)


def _stage_host_tiles(call):
    """The tiles staged through pinned buffers and uploaded on the copy stream while the overlap graph is built and the first pairs
    are registered (north star: 1.7-2.0 s of one synchronous pageable upload per tile before; streaming.upload_host_sims_async).
    The caller's images are only read; results are written to them by _write_back."""
    from .streaming import upload_host_sims_async

    call.sims_reg = upload_host_sims_async(call.sims_reg, call.device & 0xff)


def _registration_edges(call):
    """``sps``, ``affs``, ``edges``: the overlap graph of the views (mv_graph.py:35-180) and its pruning to the pairs that get
    registered (registration.py:2467-2491)."""
    from . import mv_graph

    call.sps = [si_utils.get_stack_properties_from_sim(s) for s in call.sims_reg]
    call.affs = [param_utils.select_time(si_utils.get_affine_from_sim(s, call.transform_key), 0) for s in call.sims_reg]
    tol = call.overlap_tolerance
    if tol is not None and not isinstance(tol, dict):
        tol = {d: float(tol) for d in call.sps[0]["spacing"]}
    views = [dict(sp, transform=a) for sp, a in zip(call.sps, call.affs)]
    pruning = (call.pre_registration_pruning_method, call.pre_reg_pruning_method_kwargs)
    # axis-aligned views + the default pruning: graph, overlap volumes and pruning in one library call (host code)
    call.edges = mv_graph.registration_edges_native(views, tol, call.pairs, *pruning) if _native_graph[0] else None
    if call.edges is None:
        g_views = mv_graph.build_view_adjacency_graph(views, overlap_tolerance=tol, pairs=call.pairs)
        g_views = mv_graph.prune_view_adjacency_graph(g_views, *pruning)
        call.edges = [tuple(sorted(e)) for e in g_views.edges()]


def _field_at(call, s, it):
    """Image ``s`` at time point ``it``: a shallow copy with its OWN transforms dict, so that the caller's images are never modified
    (t-stacked affines of an image without a t axis would otherwise collapse to one time point for good)."""
    tr = s.attrs.get("transforms", {})
    if (call.pairwise_executor is None or getattr(call.pairwise_executor, "reads_only", False)) and "t" not in s.dims \
            and all(np.ndim(v) == 2 for v in tr.values()):
        # nothing to select and the built-in pair path (also behind sharding.ShardedPairExecutor, which says so) only reads:
        # the image itself; any other user executor gets copies
        return s
    f = s.isel({"t": it}) if "t" in s.dims else s.copy()
    f.attrs["transforms"] = {k: param_utils.select_time(v, it) for k, v in tr.items()}
    return f


def _fields_at(call, it):
    """What compute_pairwise_registrations gets for time point ``it``: per view its field, or the pyramid of its fields."""
    if not call.multiscale:
        return [_field_at(call, s, it) for s in call.sims_reg]
    levels = [[_field_at(call, s, it) for s in lv] for lv in call.levels_reg]
    return [msi_utils.MultiscaleSpatialImage(fl, fl[0].attrs["transforms"]) for fl in levels]


def _kept_edges(results, do_filter, threshold):
    """Indices of the edges that go into the resolution.  mv_graph.filter_edges removes edges with quality < threshold only: a NaN
    quality (constant overlap -> identity transform) stays in the graph, as in the reference."""
    return [k for k, r in enumerate(results) if not (do_filter and r["quality"] < threshold)]


def _resolve_group(call, results, keep):
    """Groupwise resolution of one time point (registration.py:2560-2580 -> param_resolution.groupwise_resolution): (params, info)."""
    from . import param_resolution

    n, method = len(call.sims), call.groupwise_resolution_method
    edges, kept = [call.edges[k] for k in keep], [results[k] for k in keep]
    if method == "linear":
        return resolve_translations(n, edges, kept), None
    gkw = dict(call.groupwise_resolution_kwargs or {})
    if method == "global_optimization" and _native_resolution[0] and keep and \
            set(gkw) <= {"reference_view", "transform", "max_iter", "rel_tol", "abs_tol"}:
        # a connected translation mosaic whose sweeps end below abs_tol: the whole resolution in one library call (host code)
        fast = param_resolution.resolve_translations_native(n, edges, kept, [[sp["spacing"][d] for d in sp["spacing"]] for sp in call.sps],
                                                            **gkw)
        if fast is not None:
            return fast[0], fast[1]
    g = param_resolution.RegGraph(range(n), {v: call.sps[v] for v in range(n)})
    for (i, j), r in zip(edges, kept):
        g.add_edge(i, j, r["transform"], quality=r["quality"], bbox=r["bbox"])
    p_nodes, info = param_resolution.groupwise_resolution(g, method, **gkw)
    return [p_nodes[v] for v in range(n)], info


def _stack_params(call):
    """Per view its parameters: stacked over the time points when the images have a t axis."""
    stacked = "t" in call.sims_reg[0].dims
    return [np.stack([p[v] for p in call.params_t], axis=0) if stacked else call.params_t[0][v] for v in range(len(call.sims))]


def _write_back(call, params):
    """``new_transform_key`` on the caller's images: ``params`` rebased on ``transform_key``."""
    for m, p in zip(call.msims, params):
        if msi_utils.is_msim(m):
            msi_utils.set_affine_transform(m, p, transform_key=call.new_transform_key, base_transform_key=call.transform_key)
        else:
            si_utils.set_sim_affine(m, p, call.new_transform_key, base_transform_key=call.transform_key)


def _register_report(call, params):
    """What ``return_dict=True`` returns."""
    c = call.bin_cache
    stats = None if c is None else {"hits": c.hits, "misses": c.misses, "pairs_with_raw_crops": c.raw_crops,
                                    "pairs_on_reference_sequence": c.reference_pairs}
    qualities = {e: r["quality"] for e, r in zip(call.edges, call.all_results[0])}
    return {"params": params, "bin_cache_stats": stats, "groupwise_resolution": {"info": call.resolution_info},
            "pairwise_registration": {"edges": call.edges, "results": call.all_results, "metrics": {"qualities": qualities}}}


def register(msims, transform_key=None, reg_channel_index=None, reg_channel=None, new_transform_key=None,
             registration_binning=None, overlap_tolerance=0.0, pairwise_reg_func=phase_correlation_registration,
             pairwise_reg_func_kwargs=None, groupwise_resolution_method="global_optimization",
             groupwise_resolution_kwargs=None, pre_registration_pruning_method="alternating_pattern",
             pre_reg_pruning_method_kwargs=None,
             post_registration_do_quality_filter=False, post_registration_quality_threshold=0.2, pairs=None,
             n_parallel_pairwise_regs=None, pairwise_executor=None, return_dict=False, device=0, reg_res_level=None,
             overlap_bbox="closed_form", points_key="beads", prefilter_markers=False):
    """Register views to a common coordinate system (registration.register, registration.py:2227-2620).

    ``reg_res_level`` / ``registration_binning`` select the pyramid level of multiscale inputs per pair exactly as the
    reference does (registration.py:1639-1717, 2236, 2525): a level alone, a level plus the remaining binning, or -- by
    default -- the lowest level that divides the (optimal) binning.  The overlap graph is always built on scale0.

    ``points_key`` / ``prefilter_markers``: for a ``pairwise_reg_func`` that takes ``fixed_points`` / ``moving_points``
    (``registration_marker_based``): which point set of the views it gets (``msi_utils.set_point_set``) and whether the points
    are first restricted to the pair's overlap (see ``register_pair_of_msims``).

    Flow as in the reference: (1) overlap graph, (2) pairwise registrations of the selected edges,
    (3) groupwise resolution, (4) write ``new_transform_key`` (rebased on ``transform_key``).
    Accepts MultiscaleSpatialImages or SpatialImages (numpy- or DeviceArray-backed).  Host-side
    logic as in the reference: the overlap graph holds the intersection volume of every pair of nearby views (closed
    form for axis-aligned pairs, scipy's halfspace intersection otherwise) and is pruned by
    ``pre_registration_pruning_method`` (None, "alternating_pattern" (default), "shortest_paths_overlap_weighted",
    "otsu_threshold_on_overlap", "keep_axis_aligned").  The groupwise resolution is
    ``overlap_bbox``: how the overlap crop of a pair is sized.  "closed_form" (default): the intersection of the two world boxes
    of axis-aligned views in closed form -- N samples along an axis the views share exactly -- EXCEPT for the pairs on which the
    reference's own sequence (linprog feasible point + Qhull halfspace intersection, registration.py:229-239, 314-316) lands on
    N - 1: its vertices carry Qhull's round-off of ~1e-13, so ``floor((upper - lower) / spacing + 1)`` comes out as N or N - 1,
    and which one no closed form predicts.  The sequence is therefore asked once per pair geometry (~3 ms per pair, memoised: a
    register + fuse loop over one mosaic pays it in its first call; ``MVS_KNIFE_CHECK=0`` switches the question off), and only
    the N - 1 pairs (0 of 144 on the north star, 0 of 64 on C3, C1's one pair) leave the batched path for the reference's
    sequence.  "reference": that sequence for every pair (per-pair host path, no batching).
    ``param_resolution.groupwise_resolution`` (``groupwise_resolution_method``: "global_optimization" (default),
    "shortest_paths", a callable, or "linear" for the plain least-squares solve of ``resolve_translations``;
    ``groupwise_resolution_kwargs`` e.g. ``{"transform": "rigid", "reference_view": 0}``)."""
    if transform_key is None:
        raise ValueError("transform_key must be provided")
    call = _RegisterCall(
        msims=msims, transform_key=transform_key, reg_channel_index=reg_channel_index, reg_channel=reg_channel,
        new_transform_key=new_transform_key, registration_binning=registration_binning, overlap_tolerance=overlap_tolerance,
        pairwise_reg_func=pairwise_reg_func, pairwise_reg_func_kwargs=pairwise_reg_func_kwargs,
        groupwise_resolution_method=groupwise_resolution_method, groupwise_resolution_kwargs=groupwise_resolution_kwargs,
        pre_registration_pruning_method=pre_registration_pruning_method, pre_reg_pruning_method_kwargs=pre_reg_pruning_method_kwargs,
        post_registration_do_quality_filter=post_registration_do_quality_filter,
        post_registration_quality_threshold=post_registration_quality_threshold, pairs=pairs,
        n_parallel_pairwise_regs=n_parallel_pairwise_regs, pairwise_executor=pairwise_executor, return_dict=return_dict, device=device,
        reg_res_level=reg_res_level, overlap_bbox=overlap_bbox, points_key=points_key, prefilter_markers=prefilter_markers)
    _registration_channel(call)
    _pyramid_levels(call)
    if _wants_async_upload(call):
        _stage_host_tiles(call)
    _registration_edges(call)                                                                    # (1) graph
    for it in range(call.nt):
        results = compute_pairwise_registrations(                                                # (2) pairwise registrations
            _fields_at(call, it), call.edges, transform_key, registration_binning, overlap_tolerance, pairwise_reg_func,
            pairwise_reg_func_kwargs, pairwise_executor, device, host_threads=n_parallel_pairwise_regs, _bin_cache=call.bin_cache,
            reg_res_level=reg_res_level, overlap_bbox=overlap_bbox, points_key=points_key, prefilter_markers=prefilter_markers)
        keep = _kept_edges(results, post_registration_do_quality_filter, post_registration_quality_threshold)
        params_it, info = _resolve_group(call, results, keep)                                   # (3) groupwise resolution
        call.params_t.append(params_it)
        call.resolution_info.append(info)
        call.all_results.append(results)
    params = _stack_params(call)
    if new_transform_key is not None:
        _write_back(call, params)                                                                # (4) write back
    return _register_report(call, params) if return_dict else params


def get_pairs_from_sample_masks(mask_sims, transform_key="affine_manual", fused_mask_spacing=None, device=0):
    """registration.get_pairs_from_sample_masks (registration.py:3256-3292) on the GPU: the pairs of views whose binary sample
    masks overlap or touch under ``transform_key``.  Returns ``(pairs, fused_labels)``: ``masks.fuse_labels`` of the masks (spacing
    ``fused_mask_spacing``, default the first mask's) and ``masks.contact_pairs`` of that label image -- sorted ``(i, j)``, ``i < j``,
    each unordered pair once under full connectivity (``mv_graph.get_connected_labels`` states the difference from the
    reference's list).  ``pairs`` goes straight into ``register(..., pairs=pairs)``; ``masks.sample_masks`` makes the masks."""
    from . import masks

    fused_labels = masks.fuse_labels(mask_sims, transform_key, spacing=fused_mask_spacing, device=device)
    return masks.contact_pairs(fused_labels, device=device), fused_labels
