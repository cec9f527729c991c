"""Marker-based (bead) registration: the host side of ``registration.registration_marker_based``.

Reference: registration.py:595-1379 (descriptor matching after BigStitcher's RGLDM, RANSAC, optional ICP).  The nearest-
neighbour queries, the descriptor vectors and the scoring of all RANSAC hypotheses run on the GPU (``_marker_ops``: mvs_knn,
mvs_marker_descriptors, mvs_marker_score); what is left here works on a few hundred numbers: thresholds, the ratio test, the
sample index sets, the model fits, the ranking and the ICP bookkeeping.  Everything is float64.
"""

from __future__ import annotations

import itertools
import math
import warnings

import numpy as np

from . import _marker_ops as ops
from .param_resolution import _estimate_affine, _umeyama

NEAR_TIE_RTOL = 1e-12     # RANSAC hypotheses this close to the best quality are scored again on the host (see run_ransac)


def min_matches(transform_type, ndim):
    """registration.py:595-606."""
    transform_type = transform_type.lower()
    if transform_type == "translation":
        return 1
    if transform_type == "rigid":
        return ndim
    if transform_type == "affine":
        return ndim + 1
    raise ValueError(
        "Unsupported marker registration transform_type "
        f"{transform_type!r}. Expected 'translation', 'rigid', or 'affine'."
    )


# ---- model fits --------------------------------------------------------------------------------------------------------------
def fit_transform(fixed, moving, transform_type):
    """registration.py:819-864 with the project's estimators: the mean difference, Umeyama without scale (the algorithm of
    skimage's EuclideanTransform.estimate; a result with NaN is degenerate) and the least-squares affine of
    ``param_resolution._estimate_affine`` (a design matrix of rank below ndim + 1 is degenerate).  Raises ValueError."""
    fixed = np.asarray(fixed, dtype=float)
    moving = np.asarray(moving, dtype=float)
    ndim = fixed.shape[1]
    if transform_type == "translation":
        m = np.eye(ndim + 1)
        m[:ndim, ndim] = np.mean(moving - fixed, axis=0)
        return m
    if transform_type == "rigid":
        m = _umeyama(fixed, moving, False)
        if np.any(np.isnan(m)):
            raise ValueError("Rigid marker registration points are degenerate.")
        return m
    if transform_type == "affine":
        design = np.concatenate([fixed, np.ones((len(fixed), 1))], axis=1)
        if np.linalg.matrix_rank(design) < ndim + 1:
            raise ValueError("Affine marker registration points are degenerate.")
        return _estimate_affine(fixed, moving)
    raise ValueError(
        "Unsupported marker registration transform_type "
        f"{transform_type!r}. Expected 'translation', 'rigid', or 'affine'."
    )


def fit_transforms_batch(fixed, moving, transform_type):
    """``fit_transform`` for S samples at once: ``fixed`` / ``moving`` are (S, m, ndim).  Returns ``(affines (S, ndim + 1,
    ndim + 1), valid (S,) bool)``; a degenerate sample has valid == False."""
    fixed = np.asarray(fixed, dtype=float)
    moving = np.asarray(moving, dtype=float)
    n_s, m, ndim = fixed.shape
    out = np.tile(np.eye(ndim + 1), (n_s, 1, 1))
    if transform_type == "translation":
        out[:, :ndim, ndim] = np.mean(moving - fixed, axis=1)
        return out, np.ones(n_s, dtype=bool)
    if transform_type == "rigid":
        src_mean, dst_mean = fixed.mean(axis=1), moving.mean(axis=1)
        src_d, dst_d = fixed - src_mean[:, None, :], moving - dst_mean[:, None, :]
        a = np.matmul(np.swapaxes(dst_d, 1, 2), src_d) / m
        valid = np.all(np.isfinite(a), axis=(1, 2))
        a = np.where(valid[:, None, None], a, 0.0)
        d = np.ones((n_s, ndim))
        d[np.linalg.det(a) < 0, ndim - 1] = -1
        u, _, v = np.linalg.svd(a)
        rank = np.linalg.matrix_rank(a)
        flip = (rank == ndim - 1) & ~(np.linalg.det(u) * np.linalg.det(v) > 0)
        keep = (rank == ndim - 1) & ~flip
        d[flip, ndim - 1] = -1
        d[keep] = 1.0
        rot = np.matmul(u * d[:, None, :], v)
        out[:, :ndim, :ndim] = rot
        out[:, :ndim, ndim] = dst_mean - np.einsum("sij,sj->si", rot, src_mean)
        valid &= rank > 0
        valid &= ~np.any(np.isnan(out), axis=(1, 2))
        return out, valid
    if transform_type == "affine":
        design = np.concatenate([fixed, np.ones((n_s, m, 1))], axis=2)
        valid = np.all(np.isfinite(design), axis=(1, 2)) & np.all(np.isfinite(moving), axis=(1, 2))
        design = np.where(valid[:, None, None], design, 0.0)
        valid &= np.linalg.matrix_rank(design) >= ndim + 1
        sol = np.matmul(np.linalg.pinv(design), np.where(valid[:, None, None], moving, 0.0))      # (S, ndim + 1, ndim)
        out[:, :ndim, :ndim] = np.swapaxes(sol[:, :ndim, :], 1, 2)
        out[:, :ndim, ndim] = sol[:, ndim, :]
        return out, valid
    raise ValueError(
        "Unsupported marker registration transform_type "
        f"{transform_type!r}. Expected 'translation', 'rigid', or 'affine'."
    )


def transform_pts(pts, affine):
    """transformation.transform_pts as the reference evaluates it (transformation.py:151-161): one ``np.dot(affine, point)``
    per point.  At world coordinates of 1e6 the rounding of another evaluation order (one matrix product) shows in the
    residuals, and through them in the quality, at 1e-12; this way the host numbers are the reference's bit for bit."""
    pts = np.asarray(pts, dtype=float)
    pts = np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1)
    affine = np.asarray(affine, dtype=float)
    return np.array([np.dot(affine, pt) for pt in pts]).reshape(len(pts), pts.shape[1])[:, :-1]


def score_host(affine, fixed, moving, max_error):
    """registration.py:867-871."""
    residuals = np.linalg.norm(transform_pts(fixed, affine) - moving, axis=1)
    return residuals, residuals <= max_error


# ---- descriptors and matching ------------------------------------------------------------------------------------------------
def nearest_neighbor_scale(point_sets, device=0):
    """registration.py:613-627: the median distance of a point to its nearest other point over all sets (mvs_knn with k = 2)."""
    nearest = []
    for points in point_sets:
        if points.shape[0] < 2:
            continue
        _, dist = ops.knn(points, points, 2, device)
        nearest.append(dist[:, 1])
    nearest = np.concatenate(nearest) if nearest else np.empty(0)
    nearest = nearest[np.isfinite(nearest)]
    return float(np.median(nearest)) if nearest.size else 0.0


def neighbor_table(indices, required):
    """registration.py:667-671 for all points at once: every row of a kNN table of a set against itself without the row's own
    index (removed by index, not by position: with duplicate points the first hit need not be the point itself), cut to the
    first ``required`` entries."""
    indices = np.asarray(indices)
    other = indices != np.arange(len(indices))[:, None]
    order = np.argsort(~other, axis=1, kind="stable")[:, :required]
    return np.take_along_axis(indices, order, axis=1)


def build_descriptors(points, num_neighbors, redundancy, device=0, out_on_device=True):
    """registration.py:653-708: ``(vectors (n * C, L), point_index (n * C,))``; ``points`` is a resident (n, ndim) set."""
    n = points.shape[0]
    required = num_neighbors + redundancy
    idx, _ = ops.knn(points, points, min(n, required + 2), device)
    vectors = ops.descriptors(points, neighbor_table(idx, required), num_neighbors, redundancy, device, out_on_device=out_on_device)
    return vectors, np.repeat(np.arange(n), math.comb(required, num_neighbors))


def candidates_from_knn(nearest_distances, nearest_indices, fixed_point_indices, moving_point_indices, descriptor_ratio,
                        descriptor_distance_threshold):
    """The loop of registration.py:753-792 without a per-descriptor Python loop.  A fixed descriptor proposes (its point, the
    moving point of its nearest moving descriptor) when that distance is below the threshold and, times the ratio, below the
    distance to the first neighbour that belongs to ANOTHER moving point (+inf when the row has none).  The result lists every
    proposed pair once, in the order of its first proposal -- the order RANSAC samples from."""
    nearest_distances = np.asarray(nearest_distances, dtype=float)
    nearest_indices = np.asarray(nearest_indices)
    moving_point_indices = np.asarray(moving_point_indices)
    best_distance = nearest_distances[:, 0]
    row_points = moving_point_indices[nearest_indices]
    best_point = row_points[:, 0]
    other = row_points != best_point[:, None]
    first_other = np.argmax(other, axis=1)
    second = np.where(other.any(axis=1), nearest_distances[np.arange(len(nearest_distances)), first_other], np.inf)
    accepted = (best_distance < descriptor_distance_threshold) & (best_distance * descriptor_ratio < second)
    pairs = np.stack([np.asarray(fixed_point_indices)[accepted], best_point[accepted]], axis=1).astype(int)
    if not len(pairs):
        return np.empty((0, 2), dtype=int)
    _, first = np.unique(pairs, axis=0, return_index=True)
    return pairs[np.sort(first)]


def match_descriptors(fixed_vectors, fixed_point_indices, moving_vectors, moving_point_indices, descriptor_ratio,
                      descriptor_distance_threshold, device=0):
    """registration.py:711-816: mvs_knn of the fixed descriptors against the moving ones, then ``candidates_from_knn``."""
    n_moving = moving_vectors.shape[0]
    query_k = min(n_moving, int(np.max(np.bincount(moving_point_indices))) + 1)
    idx, dist = ops.knn(moving_vectors, fixed_vectors, query_k, device)
    return candidates_from_knn(dist, idx, fixed_point_indices, moving_point_indices, descriptor_ratio, descriptor_distance_threshold)


def marker_candidates(fixed_points, moving_points, num_neighbors=3, redundancy=1, descriptor_ratio=3.0,
                      descriptor_distance_threshold=None, descriptor_threshold_scale=1.0, device=0):
    """The candidate correspondences (C, 2) of two point sets and the descriptor threshold used (registration.py:1312-1340)."""
    fixed_dev = ops.to_device(fixed_points, device)
    moving_dev = ops.to_device(moving_points, device)
    if descriptor_distance_threshold is None:
        scale = nearest_neighbor_scale([fixed_dev, moving_dev], device)
        descriptor_distance_threshold = float(scale * np.sqrt(math.comb(num_neighbors + 1, 2)) * descriptor_threshold_scale)
    fixed_vec, fixed_idx = build_descriptors(fixed_dev, num_neighbors, redundancy, device)
    moving_vec, moving_idx = build_descriptors(moving_dev, num_neighbors, redundancy, device)
    pairs = match_descriptors(fixed_vec, fixed_idx, moving_vec, moving_idx, descriptor_ratio, descriptor_distance_threshold, device)
    return pairs, descriptor_distance_threshold, moving_dev


# ---- RANSAC ------------------------------------------------------------------------------------------------------------------
def ransac_samples(num_candidates, min_model_matches, ransac_num_iterations, random_state):
    """The sample index sets of registration.py:910-929 as an (S, m) array: every combination when there are at most
    ``ransac_num_iterations`` of them, else one ``rng.choice(C, size=m, replace=False)`` per iteration."""
    rng = np.random.default_rng(random_state)
    if math.comb(num_candidates, min_model_matches) <= ransac_num_iterations:
        samples = list(itertools.combinations(range(num_candidates), min_model_matches))
    else:
        samples = [rng.choice(num_candidates, size=min_model_matches, replace=False) for _ in range(ransac_num_iterations)]
    return np.asarray(samples, dtype=int).reshape(len(samples), min_model_matches)


def _quality(num_inliers, mean_residual, num_candidates, max_error):
    return (num_inliers / num_candidates) * max(0.0, 1.0 - mean_residual / max_error)


def run_ransac(fixed_points, moving_points, candidate_pairs, transform_type, ransac_max_error, ransac_min_inlier_ratio,
               ransac_min_inlier_factor, ransac_num_iterations, random_state, device=0):
    """registration.py:874-1061.  All samples are fitted in one batched call and scored by one mvs_marker_score launch; the
    ranking key is the reference's (quality, inliers, -mean residual), the first best wins.  The device sums residuals in
    another order than numpy's mean, so every hypothesis whose quality lies within NEAR_TIE_RTOL (relative) of the best is
    scored again on the host before the winner is chosen.  Returns (affine, quality, inlier mask over the candidates)."""
    ndim = fixed_points.shape[1]
    min_model_matches = min_matches(transform_type, ndim)
    min_inliers = max(min_model_matches, int(np.round(min_model_matches * ransac_min_inlier_factor)))
    num_candidates = len(candidate_pairs)
    if num_candidates < min_inliers:
        raise ValueError(
            "Not enough marker correspondences for RANSAC. "
            f"Need at least {min_inliers}, got {num_candidates}."
        )
    fixed_candidates = fixed_points[candidate_pairs[:, 0]]
    moving_candidates = moving_points[candidate_pairs[:, 1]]
    samples = ransac_samples(num_candidates, min_model_matches, ransac_num_iterations, random_state)
    affines, valid = fit_transforms_batch(fixed_candidates[samples], moving_candidates[samples], transform_type)
    affines = affines[valid]
    if not len(affines):
        raise ValueError("No marker transform model could be estimated.")
    counts, sums = ops.score(affines, fixed_candidates, moving_candidates, ransac_max_error, device)
    counts = counts.astype(int)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = np.where(counts > 0, sums / np.maximum(counts, 1), np.inf)
        qualities = np.where(counts > 0, (counts / num_candidates) * np.maximum(0.0, 1.0 - means / ransac_max_error), 0.0)
    best_q = float(np.max(qualities))
    near = np.flatnonzero(qualities >= best_q - NEAR_TIE_RTOL * max(best_q, np.finfo(float).tiny))
    keys = []
    for h in near:       # (usually one hypothesis, whose inlier mask is needed anyway)
        residuals, mask = score_host(affines[h], fixed_candidates, moving_candidates, ransac_max_error)
        n_in = int(np.sum(mask))
        mean_residual = float(np.mean(residuals[mask])) if n_in else np.inf
        keys.append(((_quality(n_in, mean_residual, num_candidates, ransac_max_error) if n_in else 0.0, n_in, -mean_residual), mask))
    best = max(range(len(near)), key=lambda i: keys[i][0])      # max() keeps the first of equal keys, like the reference's `>`
    inlier_mask = keys[best][1]
    num_inliers = int(np.sum(inlier_mask))
    inlier_ratio = num_inliers / num_candidates
    if num_inliers < min_inliers or inlier_ratio < ransac_min_inlier_ratio:
        raise ValueError(
            "Marker RANSAC did not find enough inliers. "
            f"Found {num_inliers}/{num_candidates} inliers."
        )
    affine = fit_transform(fixed_candidates[inlier_mask], moving_candidates[inlier_mask], transform_type)
    residuals, inlier_mask = score_host(affine, fixed_candidates, moving_candidates, ransac_max_error)
    num_inliers = int(np.sum(inlier_mask))
    if num_inliers < min_inliers:
        raise ValueError(
            "Refit marker transform did not preserve enough inliers. "
            f"Found {num_inliers}/{num_candidates} inliers."
        )
    mean_residual = float(np.mean(residuals[inlier_mask]))
    return affine, _quality(num_inliers, mean_residual, num_candidates, ransac_max_error), inlier_mask


def run_icp(fixed_points, moving_points, moving_resident, initial_affine, initial_quality, transform_type, icp_max_error,
            icp_num_iterations, icp_tolerance, device=0):
    """registration.py:1064-1145: one mvs_knn (k = 1) against the resident moving points per iteration; the fit, the quality and
    the stopping rules on the host."""
    affine = np.asarray(initial_affine, dtype=float)
    ndim = fixed_points.shape[1]
    need = min_matches(transform_type, ndim)
    quality = float(initial_quality)
    for _ in range(icp_num_iterations):
        idx, dist = ops.knn(moving_resident, transform_pts(fixed_points, affine), 1, device)
        nearest_indices, nearest_distances = idx[:, 0], dist[:, 0]
        inlier_mask = nearest_distances <= icp_max_error
        num_inliers = int(np.sum(inlier_mask))
        if num_inliers < need:
            break
        try:
            next_affine = fit_transform(fixed_points[inlier_mask], moving_points[nearest_indices[inlier_mask]], transform_type)
        except ValueError:
            break
        mean_residual = float(np.mean(nearest_distances[inlier_mask]))
        quality = _quality(num_inliers, mean_residual, len(fixed_points), icp_max_error)
        affine_delta = float(np.linalg.norm(next_affine - affine))
        affine = next_affine
        if affine_delta <= icp_tolerance:
            break
    return affine, quality


# ---- the entry point -----------------------------------------------------------------------------------------------------------
def _fail(ndim, message, fail_on_error):
    """registration.py:1148-1162."""
    if fail_on_error:
        raise ValueError(message)
    warnings.warn(message, UserWarning, stacklevel=4)
    return {"affine_matrix": np.eye(ndim + 1), "quality": np.nan}


def validate(fixed_points, moving_points, transform_type, num_neighbors, redundancy, descriptor_ratio, descriptor_distance_threshold,
             descriptor_threshold_scale, ransac_max_error, ransac_num_iterations, icp_max_error, icp_num_iterations, icp_tolerance):
    """The argument checks of registration.py:1274-1322 and :656-660, in the reference's order and words (ValueError), then
    the limits of the kernels (NotImplementedError).  Touches no device.  Returns (transform_type, icp_max_error)."""
    if fixed_points.ndim != 2 or moving_points.ndim != 2:
        raise ValueError("Marker point arrays must be two-dimensional.")
    if fixed_points.shape[1] != moving_points.shape[1]:
        raise ValueError("Fixed and moving marker points must have the same dimensionality.")
    if not len(fixed_points) or not len(moving_points):
        raise ValueError("Marker point arrays must not be empty.")
    if num_neighbors < 1:
        raise ValueError("num_neighbors must be at least 1.")
    if redundancy < 0:
        raise ValueError("redundancy must be non-negative.")
    if descriptor_ratio <= 0:
        raise ValueError("descriptor_ratio must be positive.")
    if descriptor_threshold_scale < 0:
        raise ValueError("descriptor_threshold_scale must be non-negative.")
    if ransac_max_error <= 0:
        raise ValueError("ransac_max_error must be positive.")
    if ransac_num_iterations < 1:
        raise ValueError("ransac_num_iterations must be at least 1.")
    if icp_max_error is None:
        icp_max_error = ransac_max_error
    elif icp_max_error <= 0:
        raise ValueError("icp_max_error must be positive.")
    if icp_num_iterations < 1:
        raise ValueError("icp_num_iterations must be at least 1.")
    if icp_tolerance < 0:
        raise ValueError("icp_tolerance must be non-negative.")
    transform_type = str(transform_type).lower()
    min_matches(transform_type, fixed_points.shape[1])
    if descriptor_distance_threshold is not None and descriptor_distance_threshold < 0:
        raise ValueError("descriptor_distance_threshold must be non-negative.")
    required = num_neighbors + redundancy
    for points in (fixed_points, moving_points):
        if len(points) < required + 1:
            raise ValueError(
                "Not enough points to build marker descriptors. "
                f"Need at least {required + 1}, got {len(points)}."
            )
    if fixed_points.shape[1] not in (2, 3):
        raise NotImplementedError(f"ndim = {fixed_points.shape[1]}: marker registration takes 2-D or 3-D points")
    ops.check_descriptor_params(int(num_neighbors), int(redundancy))
    return transform_type, icp_max_error


def register_details(fixed_points, moving_points, transform_type="rigid", num_neighbors=3, redundancy=1, descriptor_ratio=3.0,
                     descriptor_distance_threshold=None, descriptor_threshold_scale=1.0, ransac_max_error=5.0,
                     ransac_min_inlier_ratio=0.1, ransac_min_inlier_factor=3.0, ransac_num_iterations=1000, icp=False,
                     icp_max_error=None, icp_num_iterations=50, icp_tolerance=1e-6, random_state=0, device=0):
    """The body of registration.py:1274-1365 (raises ValueError on every failure).  Returns the result dict plus
    ``candidate_pairs`` (C, 2), ``inlier_mask`` (the refit's, over the candidates) and ``descriptor_distance_threshold``."""
    fixed_points = np.asarray(fixed_points, dtype=float)
    moving_points = np.asarray(moving_points, dtype=float)
    transform_type, icp_max_error = validate(fixed_points, moving_points, transform_type, num_neighbors, redundancy, descriptor_ratio,
                                             descriptor_distance_threshold, descriptor_threshold_scale, ransac_max_error,
                                             ransac_num_iterations, icp_max_error, icp_num_iterations, icp_tolerance)
    pairs, threshold, moving_dev = marker_candidates(fixed_points, moving_points, int(num_neighbors), int(redundancy), descriptor_ratio,
                                                     descriptor_distance_threshold, descriptor_threshold_scale, device)
    if len(pairs) == 0:
        raise ValueError("No marker correspondence candidates found.")
    affine, quality, inlier_mask = run_ransac(fixed_points, moving_points, pairs, transform_type, ransac_max_error,
                                              ransac_min_inlier_ratio, ransac_min_inlier_factor, ransac_num_iterations, random_state, device)
    if icp:
        affine, quality = run_icp(fixed_points, moving_points, moving_dev, affine, quality, transform_type, icp_max_error,
                                  icp_num_iterations, icp_tolerance, device)
    return {"affine_matrix": affine, "quality": quality, "candidate_pairs": pairs, "inlier_mask": inlier_mask,
            "descriptor_distance_threshold": threshold}


def registration_marker_based(fixed_points, moving_points, fail_on_error=True, **kwargs):
    fixed_points = np.asarray(fixed_points, dtype=float)
    moving_points = np.asarray(moving_points, dtype=float)
    if fixed_points.ndim == 2:
        ndim = fixed_points.shape[1]
    elif moving_points.ndim == 2:
        ndim = moving_points.shape[1]
    else:
        ndim = 2
    try:
        res = register_details(fixed_points, moving_points, **kwargs)
    except ValueError as exc:
        return _fail(ndim, str(exc), fail_on_error)
    return {"affine_matrix": res["affine_matrix"], "quality": res["quality"]}
