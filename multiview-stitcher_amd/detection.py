"""Bead detection: the reference's ``detection.log_detect`` / ``detection.detect_beads`` (src/multiview_stitcher/detection.py)
with the per-voxel work on the GPU.

The Laplacian-of-Gaussian response, the box maximum, the comparisons and the neighbourhood-minimum rule run in two library
calls (``_detect_ops.log_response`` / ``local_maxima``); what comes back from the device is the list of detected voxels.  The
connected-component labelling and the centres of mass are host work on that list (``label_sparse`` / ``sparse_centroids``): a
label volume is only built where a caller asks for one (``log_detect``'s contract)."""

from __future__ import annotations

import numpy as np

from . import _detect_ops, msi_utils
from . import spatial_image_utils as si_utils
from .device import DeviceArray, is_device_array


# ---- parameters ---------------------------------------------------------------------------------------------------------------
def _normalize_target_size_physical(target_size_physical, ndim):
    if isinstance(target_size_physical, bool):
        raise TypeError("target_size_physical must be a float or dict[str, float].")
    if isinstance(target_size_physical, (int, float, np.integer, np.floating)):
        return tuple(float(target_size_physical) for _ in range(ndim))
    if isinstance(target_size_physical, dict):
        if len(target_size_physical) != ndim or not all(isinstance(dim, str) for dim in target_size_physical):
            raise TypeError("target_size_physical must be a float or dict[str, float].")
        return tuple(float(size) for size in target_size_physical.values())
    raise TypeError("target_size_physical must be a float or dict[str, float].")


def _target_size_pixels(target_size_physical, spacing):
    spacing = tuple(float(sp) for sp in spacing)
    sizes = _normalize_target_size_physical(target_size_physical, len(spacing))
    return tuple(size / sp for size, sp in zip(sizes, spacing))


def log_detect_parameters(spacing, target_size_physical):
    """(sigma, minimum distance, maximum-filter size) per axis, in pixels, as the reference derives them:
    sigma = max(0.5, size / (2 sqrt(ndim))), distance = max(1, size / 2), window = 2 ceil(distance) + 1."""
    target = _target_size_pixels(target_size_physical, spacing)
    ndim = len(target)
    sigma = tuple(max(0.5, size / (2.0 * np.sqrt(ndim))) for size in target)
    min_distance = tuple(max(1.0, size / 2.0) for size in target)
    window = tuple(2 * int(np.ceil(d)) + 1 for d in min_distance)
    return sigma, min_distance, window


def _log_detect_required_overlap(kwargs):
    sigma, min_distance, _ = log_detect_parameters(kwargs["spacing"], kwargs["target_size_physical"])
    return tuple(max(1, int(np.ceil(4 * s + d))) for s, d in zip(sigma, min_distance))


def _neighbourhood_rule(spacing, target_size_physical, max_neigh_sample_size, max_neigh_sigma, ndim):
    """(window sizes of the minimum filter, sigma of the smoothing in pixels or None).  scipy truncates a filter size to int."""
    physical = _normalize_target_size_physical(target_size_physical if max_neigh_sample_size is None else max_neigh_sample_size, ndim)
    sizes = tuple(int(p / float(sp)) for p, sp in zip(physical, spacing))
    if min(sizes) < 1:
        raise ValueError(f"the neighbourhood of max_neigh_intensity has no extent in pixels: {sizes}")
    sigma = None
    if max_neigh_sigma is not None:
        sigma = tuple(s / float(sp) for s, sp in zip(_normalize_target_size_physical(max_neigh_sigma, ndim), spacing))
    return sizes, sigma


# ---- labelling a sparse set of voxels -------------------------------------------------------------------------------------------
def label_sparse(coords, shape):
    """Labels (1-based, one per row) of the voxels ``coords`` ((n, ndim) integers in raster order, no duplicates) as
    ``scipy.ndimage.label`` numbers them in a volume of ``shape``: face connectivity, components numbered in raster order of their
    first voxel.  Minimum-index propagation over the face-neighbour pairs with pointer jumping; the pairs come from a search in
    the sorted linear indices."""
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, len(shape))
    n = len(coords)
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    keys = np.ravel_multi_index(tuple(coords.T), shape)
    if np.any(np.diff(keys) <= 0):
        raise ValueError("coords must be in raster order without duplicates")
    strides = np.cumprod((1,) + tuple(shape[:0:-1]))[::-1]
    first, second = [], []
    for ax in range(len(shape)):
        src = np.nonzero(coords[:, ax] + 1 < shape[ax])[0]
        want = keys[src] + strides[ax]
        pos = np.searchsorted(keys, want)
        hit = (pos < n) & (keys[np.minimum(pos, n - 1)] == want)
        first.append(src[hit])
        second.append(pos[hit])
    a, b = np.concatenate(first), np.concatenate(second)
    root = np.arange(n)
    while True:
        new = root.copy()
        low = np.minimum(root[a], root[b])
        np.minimum.at(new, a, low)
        np.minimum.at(new, b, low)
        new = new[new]
        if np.array_equal(new, root):
            break
        root = new
    return (np.searchsorted(np.unique(root), root) + 1).astype(np.int32)


def sparse_centroids(coords, labels):
    """(n_labels, ndim) float64: the mean voxel index of every label, in label order -- what
    ``scipy.ndimage.center_of_mass(labels, labels, ids)`` yields for a label volume."""
    coords = np.asarray(coords, dtype=np.float64)
    if len(coords) == 0:
        return np.empty((0, coords.shape[1] if coords.ndim == 2 else 0), dtype=np.float64)
    ids = np.asarray(labels, dtype=np.int64) - 1
    counts = np.bincount(ids)
    return np.stack([np.bincount(ids, weights=coords[:, k]) / counts for k in range(coords.shape[1])], axis=1)


def _dense_label_centroids(labels):
    """Centroids of an integer label volume (a custom detection function's result), in label order."""
    if not np.issubdtype(np.asarray(labels).dtype, np.integer):
        raise TypeError("detection_func must return an integer label array.")
    labels = np.asarray(labels)
    coords = np.argwhere(labels > 0)
    if len(coords) == 0:
        return np.empty((0, labels.ndim), dtype=np.float64)
    _, dense = np.unique(labels[labels > 0], return_inverse=True)
    return sparse_centroids(coords, np.asarray(dense).reshape(-1) + 1)


# ---- detection on one block ---------------------------------------------------------------------------------------------------
def _detect_sparse(image, spacing, target_size_physical, threshold_rel=0.2, threshold_abs=None, max_neigh_intensity=None,
                   max_neigh_sample_size=None, max_neigh_sigma=None, device=0, response_max=None):
    """The detected voxels of one block, (n, ndim) int64 in raster order.  ``response_max``: the maximum ``threshold_rel`` refers
    to when it is not this block's own (slabs of a larger field)."""
    ndim = len(image.shape)
    if len(tuple(spacing)) != ndim:
        raise ValueError("spacing and target_size_physical must match image.ndim.")
    sigma, _, window = log_detect_parameters(spacing, target_size_physical)
    if len(sigma) != ndim:
        raise ValueError("spacing and target_size_physical must match image.ndim.")
    rule = None
    if max_neigh_intensity is not None:
        rule = _neighbourhood_rule(spacing, target_size_physical, max_neigh_sample_size, max_neigh_sigma, ndim)
        if not is_device_array(image):      # the rule reads the image a second time: one upload for both
            image = DeviceArray.from_host(image, device)
    response, own_max = _detect_ops.log_response(image, sigma, float(np.mean(sigma)) ** 2, device=device)
    if threshold_abs is None:
        # (float32 maximum times a Python float: float32, as in the reference)
        threshold_abs = np.float32(own_max if response_max is None else response_max) * threshold_rel
    sample = sample_window = None
    if rule is not None:
        sample_window, neigh_sigma = rule
        sample = image if neigh_sigma is None else _detect_ops.gaussian_smooth(image, neigh_sigma, device=device)
    return _detect_ops.local_maxima(response, window, threshold_abs, sample, sample_window, max_neigh_intensity, device=device)


def log_detect(image, spacing, target_size_physical, threshold_rel=0.2, threshold_abs=None, max_neigh_intensity=None,
               max_neigh_sample_size=None, max_neigh_sigma=None, device=0):
    """Detect bright beads by a Laplacian-of-Gaussian (the reference's ``log_detect`` on the GPU).

    ``image``: 2-D or 3-D uint8 / uint16 / float32, a numpy array or a ``DeviceArray``; ``spacing``: pixel spacing per axis;
    ``target_size_physical``: expected bead diameter, a number or a dict per axis.  A voxel is a detection where the response
    ``-gaussian_laplace(image, sigma) * mean(sigma)^2`` equals its maximum over the window ``2 ceil(max(1, size / 2)) + 1``, exceeds
    ``threshold_abs`` (default: ``threshold_rel`` times the response maximum) and 0; with ``max_neigh_intensity`` the minimum of the
    image (smoothed by ``max_neigh_sigma`` when given) over a box of ``max_neigh_sample_size`` (default: the target size) must lie
    below it.  A box size is truncated to whole pixels as scipy does; one that truncates to 0 raises ``ValueError``.

    Returns an int32 label array of the image's shape, numbered as ``scipy.ndimage.label`` numbers the detections (face
    connectivity, raster order of each component's first voxel).  The array is a zero volume with the labels of the detected
    voxels written in; ``detect_beads`` never builds it.

    Float images that contain NaN are not supported."""
    coords = _detect_sparse(image, spacing, target_size_physical, threshold_rel, threshold_abs, max_neigh_intensity,
                            max_neigh_sample_size, max_neigh_sigma, device)
    shape = tuple(int(s) for s in image.shape)
    out = np.zeros(shape, dtype=np.int32)
    if len(coords):
        out[tuple(coords.T)] = label_sparse(coords, shape)
    return out


log_detect.required_overlap = _log_detect_required_overlap


# ---- detection on a multiscale image --------------------------------------------------------------------------------------------
def _slabs(n0, core, overlap):
    """[(core lo, core hi, slab lo, slab hi)] along the first axis: cores of ``core`` slices, extended by ``overlap`` inside [0, n0)."""
    return [(lo, min(lo + core, n0), max(lo - overlap, 0), min(min(lo + core, n0) + overlap, n0)) for lo in range(0, n0, core)]


def detect_beads(msim, detection_func=log_detect, detection_func_kwargs=None, detection_overlap=None, max_detection_spacing=None,
                 max_block_voxels=None, device=0):
    """Detect bright fiducial beads in a multiscale image (the reference's ``detect_beads``).

    Selects the resolution level (``max_detection_spacing``: the coarsest level whose spacing does not exceed it; default scale0),
    takes the first field of its non-spatial dims, applies ``detection_func`` and returns the detected positions as an
    ``(n_points, ndim)`` float64 array of ``origin + centroid * spacing`` (columns in the order of the spatial dims, rows in the order
    of the labels).  With the default ``detection_func`` the centroids come straight from the device's list of detected voxels; a
    custom function receives the numpy block and ``spacing`` and returns an integer label array, as in the reference.

    A field whose device work area does not fit, or that has more than ``max_block_voxels`` voxels (the one keyword the reference
    lacks), is processed in slabs along its first axis.  A slab extends by ``detection_overlap`` (default: the function's
    ``required_overlap``) on both sides, and a centroid counts where it falls into the slab's core, as in the reference.
    Without ``max_block_voxels`` the slabs are the thickest that fit; a budget (or a device) too small for the thinnest slab -- one
    core plane and the overlap on both sides -- raises ``ValueError`` (``MemoryError``).

    One departure from the reference: with ``threshold_rel`` the threshold refers to the response maximum of the WHOLE field (a
    first sweep over the slabs provides it), so the result does not depend on the slabs; the reference takes each chunk's own."""
    if max_detection_spacing is None:
        scale_key = "scale0"
    else:
        sdims0 = si_utils.get_spatial_dims_from_sim(msi_utils.get_sim_from_msim(msim, scale="scale0"))
        if not isinstance(max_detection_spacing, dict):
            max_detection_spacing = {d: float(max_detection_spacing) for d in sdims0}
        scale_key = f"scale{msi_utils.get_res_level_from_spacing(msim, max_detection_spacing)}"
    sim = si_utils.get_sim_field(msi_utils.get_sim_from_msim(msim, scale=scale_key))
    sdims = si_utils.get_spatial_dims_from_sim(sim)
    ndim = len(sdims)
    spacing = si_utils.get_spacing_from_sim(sim)
    spacing_tuple = tuple(spacing[d] for d in sdims)
    origin = si_utils.get_origin_from_sim(sim)
    kwargs = dict(detection_func_kwargs) if detection_func_kwargs is not None else {}

    if detection_overlap is not None and not isinstance(detection_overlap, (int, dict)):
        raise TypeError(f"detection_overlap must be an int, a dict, or None; got {type(detection_overlap).__name__}.")
    if detection_overlap is None and hasattr(detection_func, "required_overlap"):
        required = detection_func.required_overlap(kwargs | {"spacing": spacing_tuple})
        detection_overlap = required if isinstance(required, dict) else dict(zip(sdims, required))
    if detection_overlap is None:
        detection_overlap = 0
    if not isinstance(detection_overlap, dict):
        detection_overlap = {d: detection_overlap for d in sdims}
    overlap0 = int(np.ceil(detection_overlap[sdims[0]]))

    data = sim.data
    shape = tuple(int(s) for s in data.shape)
    n_voxels = int(np.prod(shape))
    default = detection_func is log_detect
    plane = n_voxels // shape[0]
    min_planes = min(2 * overlap0 + 1, shape[0])      # the thinnest slab: one core plane and its overlap
    if max_block_voxels is not None:
        whole = n_voxels <= int(max_block_voxels)
        planes = int(max_block_voxels) // plane
        if not whole and planes < min_planes:
            raise ValueError(f"max_block_voxels = {int(max_block_voxels)} is less than the thinnest slab of this field: {min_planes} planes "
                             f"(one core plane and an overlap of {overlap0} on both sides) of {plane} voxels")
    else:
        on_host = not is_device_array(data)
        fits = lambda n_planes: _detect_ops.fits_device(n_planes * plane, data.dtype.itemsize, on_host, device)      # noqa: E731
        whole = not default or fits(shape[0])
        if not whole:
            if not fits(min_planes):
                raise MemoryError(f"detect_beads: the thinnest slab of this field ({min_planes} planes of {plane} voxels: one core plane and an "
                                  f"overlap of {overlap0} on both sides) does not fit into the free device memory")
            planes, too_many = min_planes, shape[0]      # the thickest slab that fits, by bisection
            while too_many - planes > 1:
                mid = (planes + too_many) // 2
                planes, too_many = (mid, too_many) if fits(mid) else (planes, mid)
    if whole:
        slabs = [(0, shape[0], 0, shape[0])]
    else:
        slabs = _slabs(shape[0], planes - 2 * overlap0, overlap0)      # every slab has at most `planes` planes

    if default:
        sparse_kwargs = dict(kwargs, device=device)
        if len(slabs) > 1 and kwargs.get("threshold_abs") is None:
            sigma, _, _ = log_detect_parameters(spacing_tuple, kwargs["target_size_physical"])
            peaks = [_detect_ops.log_response(data[s0:s1], sigma, float(np.mean(sigma)) ** 2, max_range=(lo - s0, hi - s0), device=device)[1]
                     for lo, hi, s0, s1 in slabs]
            sparse_kwargs["response_max"] = np.nanmax(np.asarray(peaks, dtype=np.float32))
    points, first_voxels = [], []
    for lo, hi, s0, s1 in slabs:
        block = data[s0:s1]
        if default:
            coords = _detect_sparse(block, spacing_tuple, **sparse_kwargs)
            labels = label_sparse(coords, tuple(int(s) for s in block.shape))
            centroids = sparse_centroids(coords, labels)
            first = coords[np.unique(labels, return_index=True)[1]]       # (the list is in raster order)
        else:
            centroids = _dense_label_centroids(detection_func(np.asarray(block), spacing_tuple, **kwargs))
            first = np.zeros((len(centroids), ndim), dtype=np.int64)
        keep = (centroids[:, 0] >= lo - s0) & (centroids[:, 0] < hi - s0)
        centroids, first = centroids[keep], first[keep]
        centroids[:, 0] += s0
        first[:, 0] += s0
        points.append(centroids)
        first_voxels.append(first)
    indices = np.concatenate(points, axis=0)
    if default and len(slabs) > 1:
        # the order of the labels of the whole field: raster order of each component's first voxel
        indices = indices[np.argsort(np.ravel_multi_index(tuple(np.concatenate(first_voxels, axis=0).T), shape), kind="stable")]
    positions = np.empty((len(indices), ndim), dtype=np.float64)
    for k, d in enumerate(sdims):
        positions[:, k] = origin[d] + indices[:, k] * spacing[d]
    return positions
