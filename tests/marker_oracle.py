"""CPU restatement of the reference's marker-based registration (src/multiview_stitcher/registration.py:595-1162), for the
tests of ``registration.registration_marker_based``: numpy / scipy only, float64, written as the reference loops -- cKDTree
queries, itertools subsets, one hypothesis at a time.  No tests in here.

The model fits are the ones the project names: the mean difference, Umeyama without scale (the algorithm of
skimage's EuclideanTransform.estimate, degenerate when the result holds NaN) and a least-squares affine through
``np.linalg.lstsq`` (degenerate when the design matrix has rank below ndim + 1).  They are restated here, not imported.

Besides the results, the functions record how close their decisions were (``trace``): the smallest relative distance of any
compared pair of numbers -- descriptor distance against the threshold, ratio test, residual against the inlier bound -- and
the RANSAC keys, so that a test can tell an input that sits on a decision boundary from a wrong kernel."""
import itertools
import math

import numpy as np
from scipy.spatial import cKDTree


# ---- yardstick for mvs_knn -----------------------------------------------------------------------------------------------------
def brute_knn(ref, query, k):
    """All distances as sqrt(sum of squared differences), the k smallest per query by (distance, index); -1 / inf past n_ref."""
    ref = np.asarray(ref, dtype=np.float64)
    query = np.asarray(query, dtype=np.float64)
    dist = np.sqrt(((query[:, None, :] - ref[None, :, :]) ** 2).sum(axis=2))
    idx = np.empty((len(query), k), dtype=np.int32)
    out = np.empty((len(query), k), dtype=np.float64)
    index = np.arange(len(ref))
    for q in range(len(query)):
        order = np.lexsort((index, dist[q]))[:k]
        n = len(order)
        idx[q, :n], out[q, :n] = order, dist[q, order]
        idx[q, n:], out[q, n:] = -1, np.inf
    return idx, out


def _margin(trace, name, a, b):
    """Record |a - b| / max(|a|, |b|) of a comparison of two finite numbers."""
    if trace is None or not (np.isfinite(a) and np.isfinite(b)):
        return
    scale = max(abs(a), abs(b))
    m = abs(a - b) / scale if scale > 0 else 0.0
    trace[name] = min(trace.get(name, np.inf), m)


def transform_pts(pts, affine):
    """transformation.py:151-161."""
    pts = np.array(pts)
    pts = np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1)
    pts_t = np.array([np.dot(np.array(affine), pt) for pt in pts])
    return pts_t[:, :-1]


def get_min_matches(transform_type, ndim):
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


def get_nearest_neighbor_scale(*point_sets):
    nearest_distances = []
    for points in point_sets:
        points = np.asarray(points, dtype=float)
        if len(points) < 2:
            continue
        distances, _ = cKDTree(points).query(points, k=2)
        nearest_distances.extend(distances[:, 1])
    nearest_distances = np.asarray(nearest_distances, dtype=float)
    nearest_distances = nearest_distances[np.isfinite(nearest_distances)]
    if nearest_distances.size == 0:
        return 0.0
    return float(np.median(nearest_distances))


def get_descriptor_distance_threshold(fixed_points, moving_points, num_neighbors, descriptor_threshold_scale):
    length = math.comb(num_neighbors + 1, 2)
    return float(get_nearest_neighbor_scale(fixed_points, moving_points) * np.sqrt(length) * descriptor_threshold_scale)


def get_descriptors(points, num_neighbors, redundancy):
    points = np.asarray(points, dtype=float)
    required_neighbors = num_neighbors + redundancy
    if len(points) < required_neighbors + 1:
        raise ValueError(
            "Not enough points to build marker descriptors. "
            f"Need at least {required_neighbors + 1}, got {len(points)}."
        )
    tree = cKDTree(points)
    query_k = min(len(points), required_neighbors + 2)
    _, neighbor_indices = tree.query(points, k=query_k)
    descriptors = []
    for point_index, point_neighbor_indices in enumerate(neighbor_indices):
        point_neighbor_indices = np.atleast_1d(point_neighbor_indices)
        point_neighbor_indices = [int(ind) for ind in point_neighbor_indices if int(ind) != point_index][:required_neighbors]
        if len(point_neighbor_indices) < required_neighbors:
            continue
        for subset in itertools.combinations(point_neighbor_indices, num_neighbors):
            descriptor_points = points[[point_index] + list(subset)]
            distances = []
            for i, j in itertools.combinations(range(len(descriptor_points)), 2):
                distances.append(np.linalg.norm(descriptor_points[i] - descriptor_points[j]))
            descriptors.append({"point_index": point_index, "vector": np.sort(np.asarray(distances, dtype=float))})
    if len(descriptors) == 0:
        raise ValueError("No marker descriptors could be built.")
    return descriptors


def descriptor_knn(fixed_descriptors, moving_descriptors):
    """The cKDTree query of registration.py:736-751: (distances, indices, fixed point indices, moving point indices)."""
    fixed_vectors = np.asarray([d["vector"] for d in fixed_descriptors], dtype=float)
    fixed_point_indices = np.asarray([d["point_index"] for d in fixed_descriptors], dtype=int)
    moving_vectors = np.asarray([d["vector"] for d in moving_descriptors], dtype=float)
    moving_point_indices = np.asarray([d["point_index"] for d in moving_descriptors], dtype=int)
    _, counts = np.unique(moving_point_indices, return_counts=True)
    query_k = min(len(moving_vectors), int(np.max(counts)) + 1)
    nearest_distances, nearest_indices = cKDTree(moving_vectors).query(fixed_vectors, k=query_k)
    nearest_distances = np.asarray(nearest_distances, dtype=float)
    nearest_indices = np.asarray(nearest_indices, dtype=int)
    if query_k == 1:
        nearest_distances = nearest_distances[:, np.newaxis]
        nearest_indices = nearest_indices[:, np.newaxis]
    return nearest_distances, nearest_indices, fixed_point_indices, moving_point_indices


def candidates_from_knn(nearest_distances, nearest_indices, fixed_point_indices, moving_point_indices, descriptor_ratio,
                        descriptor_distance_threshold, trace=None):
    """The loop of registration.py:753-792."""
    candidates_by_pair = {}
    for fixed_point_index, row_distances, row_indices in zip(fixed_point_indices, nearest_distances, nearest_indices):
        best_descriptor_index = row_indices[0]
        best_moving_point_index = moving_point_indices[best_descriptor_index]
        best_distance = float(row_distances[0])
        _margin(trace, "descriptor_threshold", best_distance, descriptor_distance_threshold)
        if not best_distance < descriptor_distance_threshold:
            continue
        row_moving_point_indices = moving_point_indices[row_indices]
        second_best_mask = row_moving_point_indices != best_moving_point_index
        if np.any(second_best_mask):
            second_best_distance = float(row_distances[np.flatnonzero(second_best_mask)[0]])
        else:
            second_best_distance = np.inf
        _margin(trace, "descriptor_ratio", best_distance * descriptor_ratio, second_best_distance)
        if best_distance * descriptor_ratio < second_best_distance:
            pair = (int(fixed_point_index), int(best_moving_point_index))
            if pair not in candidates_by_pair or best_distance < candidates_by_pair[pair]:
                candidates_by_pair[pair] = best_distance
    return np.asarray(list(candidates_by_pair.keys()), dtype=int).reshape(len(candidates_by_pair), 2)


def match_descriptors(fixed_descriptors, moving_descriptors, descriptor_ratio, descriptor_distance_threshold, trace=None):
    if len(fixed_descriptors) == 0 or len(moving_descriptors) == 0:
        return np.empty((0, 2), dtype=int)
    return candidates_from_knn(*descriptor_knn(fixed_descriptors, moving_descriptors), descriptor_ratio, descriptor_distance_threshold, trace)


# ---- fits ----------------------------------------------------------------------------------------------------------------------
def umeyama(src, dst):
    """Umeyama 1991 without scale, as skimage.transform._geometric._umeyama(src, dst, estimate_scale=False)."""
    num, dim = src.shape
    src_mean, dst_mean = src.mean(axis=0), dst.mean(axis=0)
    src_demean, dst_demean = src - src_mean, dst - dst_mean
    A = dst_demean.T @ src_demean / num
    d = np.ones((dim,), dtype=np.float64)
    if np.linalg.det(A) < 0:
        d[dim - 1] = -1
    T = np.eye(dim + 1, dtype=np.float64)
    U, S, V = np.linalg.svd(A)
    rank = np.linalg.matrix_rank(A)
    if rank == 0:
        return np.nan * T
    elif rank == dim - 1:
        if np.linalg.det(U) * np.linalg.det(V) > 0:
            T[:dim, :dim] = U @ V
        else:
            s = d[dim - 1]
            d[dim - 1] = -1
            T[:dim, :dim] = U @ np.diag(d) @ V
            d[dim - 1] = s
    else:
        T[:dim, :dim] = U @ np.diag(d) @ V
    T[:dim, dim] = dst_mean - (T[:dim, :dim] @ src_mean.T)
    return T


def fit_transform(fixed_points, moving_points, transform_type):
    fixed_points = np.asarray(fixed_points, dtype=float)
    moving_points = np.asarray(moving_points, dtype=float)
    ndim = fixed_points.shape[1]
    transform_type = transform_type.lower()
    if transform_type == "translation":
        params = np.eye(ndim + 1)
        params[:ndim, ndim] = np.mean(moving_points - fixed_points, axis=0)
        return params
    if transform_type == "rigid":
        params = umeyama(fixed_points, moving_points)
        if np.any(np.isnan(params)):
            raise ValueError("Rigid marker registration points are degenerate.")
        return params
    if transform_type == "affine":
        X = np.concatenate([fixed_points, np.ones((len(fixed_points), 1))], axis=1)
        if np.linalg.matrix_rank(X) < ndim + 1:
            raise ValueError("Affine marker registration points are degenerate.")
        sol, *_ = np.linalg.lstsq(X, moving_points, rcond=None)
        params = np.eye(ndim + 1)
        params[:ndim, :ndim] = sol[:ndim].T
        params[:ndim, ndim] = sol[ndim]
        return params
    raise ValueError(
        "Unsupported marker registration transform_type "
        f"{transform_type!r}. Expected 'translation', 'rigid', or 'affine'."
    )


def score_transform(affine, fixed_points, moving_points, ransac_max_error):
    transformed_fixed_points = transform_pts(fixed_points, affine)
    residuals = np.linalg.norm(transformed_fixed_points - moving_points, axis=1)
    return residuals, residuals <= ransac_max_error


def ransac_sample_sets(num_candidates, min_model_matches, ransac_num_iterations, random_state):
    """The sample index sets of registration.py:910-929, as a list."""
    rng = np.random.default_rng(random_state)
    if math.comb(num_candidates, min_model_matches) <= ransac_num_iterations:
        sample_iter = itertools.combinations(range(num_candidates), min_model_matches)
    else:
        sample_iter = (rng.choice(num_candidates, size=min_model_matches, replace=False) for _ in range(ransac_num_iterations))
    return [np.asarray(s, dtype=int) for s in sample_iter]


def run_ransac(fixed_points, moving_points, candidate_pairs, transform_type, ransac_max_error, ransac_min_inlier_ratio,
               ransac_min_inlier_factor, ransac_num_iterations, random_state, trace=None):
    """registration.py:874-1061; returns (affine, quality, inlier mask of the refit)."""
    ndim = fixed_points.shape[1]
    min_model_matches = get_min_matches(transform_type, ndim)
    min_inliers = max(min_model_matches, int(np.round(min_model_matches * ransac_min_inlier_factor)))
    if len(candidate_pairs) < min_inliers:
        raise ValueError(
            "Not enough marker correspondences for RANSAC. "
            f"Need at least {min_inliers}, got {len(candidate_pairs)}."
        )
    fixed_candidates = fixed_points[candidate_pairs[:, 0]]
    moving_candidates = moving_points[candidate_pairs[:, 1]]
    best_result = None
    num_candidates = len(candidate_pairs)
    keys = []
    for sample_indices in ransac_sample_sets(num_candidates, min_model_matches, ransac_num_iterations, random_state):
        try:
            affine = fit_transform(fixed_candidates[sample_indices], moving_candidates[sample_indices], transform_type)
        except ValueError:
            continue
        residuals, inlier_mask = score_transform(affine, fixed_candidates, moving_candidates, ransac_max_error)
        num_inliers = int(np.sum(inlier_mask))
        if num_inliers == 0:
            mean_residual = np.inf
            model_quality = 0.0
        else:
            mean_residual = float(np.mean(residuals[inlier_mask]))
            model_quality = (num_inliers / num_candidates) * max(0.0, 1.0 - mean_residual / ransac_max_error)
        result_key = (model_quality, num_inliers, -mean_residual)
        keys.append((result_key, residuals))
        if best_result is None or result_key > best_result["key"]:
            best_result = {"key": result_key, "inlier_mask": inlier_mask, "residuals": residuals}
    if best_result is None:
        raise ValueError("No marker transform model could be estimated.")
    if trace is not None:
        # the gap between the best key and the best key of a hypothesis with OTHER inliers, relative, in the quality; equal keys
        # of one and the same model (the same sample drawn twice, permutations of it) decide nothing
        best_q = best_result["key"][0]
        others = [k[0] for k, r in keys if k != best_result["key"] and not np.array_equal(r <= ransac_max_error, best_result["inlier_mask"])]
        trace["ransac_key_gap"] = (best_q - max(others)) / best_q if others and best_q > 0 else np.inf
        for r in best_result["residuals"]:
            _margin(trace, "inlier_bound", float(r), ransac_max_error)
    inlier_mask = best_result["inlier_mask"]
    num_inliers = int(np.sum(inlier_mask))
    inlier_ratio = num_inliers / num_candidates
    if num_inliers < min_inliers or inlier_ratio < ransac_min_inlier_ratio:
        raise ValueError(
            "Marker RANSAC did not find enough inliers. "
            f"Found {num_inliers}/{num_candidates} inliers."
        )
    affine = fit_transform(fixed_candidates[inlier_mask], moving_candidates[inlier_mask], transform_type)
    residuals, inlier_mask = score_transform(affine, fixed_candidates, moving_candidates, ransac_max_error)
    for r in residuals:
        _margin(trace, "inlier_bound", float(r), ransac_max_error)
    num_inliers = int(np.sum(inlier_mask))
    if num_inliers < min_inliers:
        raise ValueError(
            "Refit marker transform did not preserve enough inliers. "
            f"Found {num_inliers}/{num_candidates} inliers."
        )
    mean_residual = float(np.mean(residuals[inlier_mask]))
    inlier_ratio = float(num_inliers / num_candidates)
    quality = inlier_ratio * max(0.0, 1.0 - mean_residual / ransac_max_error)
    return affine, quality, inlier_mask


def run_icp(fixed_points, moving_points, initial_affine, initial_quality, transform_type, icp_max_error, icp_num_iterations,
            icp_tolerance, trace=None):
    fixed_points = np.asarray(fixed_points, dtype=float)
    moving_points = np.asarray(moving_points, dtype=float)
    affine = np.asarray(initial_affine, dtype=float)
    ndim = fixed_points.shape[1]
    min_matches = get_min_matches(transform_type, ndim)
    moving_tree = cKDTree(moving_points)
    quality = float(initial_quality)
    for _ in range(icp_num_iterations):
        transformed_fixed_points = transform_pts(fixed_points, affine)
        nearest_distances, nearest_indices = moving_tree.query(transformed_fixed_points, k=1)
        for r in nearest_distances:
            _margin(trace, "icp_bound", float(r), icp_max_error)
        inlier_mask = nearest_distances <= icp_max_error
        num_inliers = int(np.sum(inlier_mask))
        if num_inliers < min_matches:
            break
        try:
            next_affine = fit_transform(fixed_points[inlier_mask], moving_points[nearest_indices[inlier_mask]], transform_type)
        except ValueError:
            break
        mean_residual = float(np.mean(nearest_distances[inlier_mask]))
        quality = (num_inliers / len(fixed_points)) * max(0.0, 1.0 - mean_residual / icp_max_error)
        affine_delta = float(np.linalg.norm(next_affine - affine))
        affine = next_affine
        if affine_delta <= icp_tolerance:
            break
    return affine, quality


def registration_marker_based(fixed_points, moving_points, transform_type="rigid", num_neighbors=3, redundancy=1, descriptor_ratio=3.0,
                              descriptor_distance_threshold=None, descriptor_threshold_scale=1.0, ransac_max_error=5.0,
                              ransac_min_inlier_ratio=0.1, ransac_min_inlier_factor=3.0, ransac_num_iterations=1000, icp=False,
                              icp_max_error=None, icp_num_iterations=50, icp_tolerance=1e-6, random_state=0):
    """registration.py:1312-1365 for valid arguments; raises ValueError where the reference's body does.  Returns the result
    dict plus ``candidate_pairs``, ``inlier_mask`` (of the RANSAC refit) and ``trace`` (the decision margins)."""
    fixed_points = np.asarray(fixed_points, dtype=float)
    moving_points = np.asarray(moving_points, dtype=float)
    trace = {}
    if icp_max_error is None:
        icp_max_error = ransac_max_error
    transform_type = str(transform_type).lower()
    if descriptor_distance_threshold is None:
        descriptor_distance_threshold = get_descriptor_distance_threshold(fixed_points, moving_points, num_neighbors, descriptor_threshold_scale)
    fixed_descriptors = get_descriptors(fixed_points, num_neighbors, redundancy)
    moving_descriptors = get_descriptors(moving_points, num_neighbors, redundancy)
    candidate_pairs = match_descriptors(fixed_descriptors, moving_descriptors, descriptor_ratio, descriptor_distance_threshold, trace)
    if len(candidate_pairs) == 0:
        raise ValueError("No marker correspondence candidates found.")
    affine, quality, inlier_mask = run_ransac(fixed_points, moving_points, candidate_pairs, transform_type, ransac_max_error,
                                              ransac_min_inlier_ratio, ransac_min_inlier_factor, ransac_num_iterations, random_state, trace)
    if icp:
        affine, quality = run_icp(fixed_points, moving_points, affine, quality, transform_type, icp_max_error, icp_num_iterations,
                                  icp_tolerance, trace)
    return {"affine_matrix": affine, "quality": quality, "candidate_pairs": candidate_pairs, "inlier_mask": inlier_mask, "trace": trace}


def min_margin(trace):
    """The smallest relative margin of any threshold or ratio decision recorded in ``trace``."""
    return min([v for k, v in trace.items() if k != "ransac_key_gap"] or [np.inf])


# ---- test scenes ---------------------------------------------------------------------------------------------------------------
def rotation(ndim, angle):
    c, s = np.cos(angle), np.sin(angle)
    if ndim == 2:
        return np.array([[c, -s], [s, c]])
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]) @ np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def make_pair(ndim, n, seed, box=200.0, angle=0.15, shift=None, noise=0.1, drop=0.2, n_outliers=20, offset=0.0):
    """Fixed points uniform in a box; moving = rotation about the centroid + shift + noise, a share dropped, outliers added,
    rows permuted.  Returns (fixed, moving, true fixed -> moving matrix)."""
    rng = np.random.default_rng(seed)
    fixed = rng.uniform(0.0, box, size=(n, ndim)) + offset
    rot = rotation(ndim, angle)
    shift = np.array([3.0, -4.0, 2.5][:ndim]) if shift is None else np.asarray(shift, dtype=float)
    centre = fixed.mean(axis=0)
    moving = (fixed - centre) @ rot.T + centre + shift
    if noise:
        moving = moving + rng.normal(0.0, noise, size=moving.shape)
    keep = rng.random(n) >= drop
    moving = moving[keep]
    if n_outliers:
        moving = np.concatenate([moving, rng.uniform(0.0, box, size=(n_outliers, ndim)) + offset])
    moving = moving[rng.permutation(len(moving))]
    true = np.eye(ndim + 1)
    true[:ndim, :ndim] = rot
    true[:ndim, ndim] = centre + shift - rot @ centre
    return fixed, moving, true
