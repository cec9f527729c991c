"""Restatement of the reference's detection arithmetic (src/multiview_stitcher/detection.py: log_detect, and the label /
centre-of-mass step of detect_beads) with scipy, for the tests of multiview_stitcher_amd.detection, plus a seeded bead image.

``mode``: numpy.float32 is the reference's own precision (the image is filtered as float32); numpy.float64 filters the image as
float64 and is the yardstick both the float32 mode and the GPU are measured against."""
import numpy as np
from scipy import ndimage


def parameters(spacing, target_size_physical):
    """(sigma, minimum distance, maximum-filter size) per axis in pixels."""
    ndim = len(spacing)
    if isinstance(target_size_physical, dict):
        physical = [float(v) for v in target_size_physical.values()]
    else:
        physical = [float(target_size_physical)] * ndim
    size = [p / float(sp) for p, sp in zip(physical, spacing)]
    sigma = tuple(max(0.5, s / (2.0 * np.sqrt(ndim))) for s in size)
    dist = tuple(max(1.0, s / 2.0) for s in size)
    return sigma, dist, tuple(2 * int(np.ceil(d)) + 1 for d in dist)


def response(image, sigma, mode=np.float32):
    r = -ndimage.gaussian_laplace(image.astype(mode, copy=False), sigma=sigma, mode="reflect")
    r *= float(np.mean(sigma)) ** 2
    return r


def detections(resp, window, threshold_abs, image=None, max_neigh_intensity=None, min_filter_size=None, neigh_sigma=None):
    """Boolean mask of the detections in a response volume (the reference's comparisons)."""
    mask = (resp == ndimage.maximum_filter(resp, size=window, mode="reflect")) & (resp > threshold_abs) & (resp > 0)
    if max_neigh_intensity is not None:
        sample = image
        if neigh_sigma is not None:
            sample = ndimage.gaussian_filter(image.astype(np.float32, copy=False), sigma=neigh_sigma)
        mask &= ndimage.minimum_filter(sample, size=min_filter_size, mode="reflect") < max_neigh_intensity
    return mask


def log_detect(image, spacing, target_size_physical, threshold_rel=0.2, threshold_abs=None, max_neigh_intensity=None,
               max_neigh_sample_size=None, max_neigh_sigma=None, mode=np.float32, return_parts=False):
    """The reference's log_detect.  Returns the int32 label array (``return_parts``: (labels, response, mask, threshold))."""
    sigma, _, window = parameters(spacing, target_size_physical)
    resp = response(image, sigma, mode)
    if threshold_abs is None:
        threshold_abs = np.nanmax(resp) * threshold_rel
    size = neigh_sigma = None
    if max_neigh_intensity is not None:
        src = target_size_physical if max_neigh_sample_size is None else max_neigh_sample_size
        physical = [float(v) for v in src.values()] if isinstance(src, dict) else [float(src)] * image.ndim
        size = [p / float(sp) for p, sp in zip(physical, spacing)]
        if max_neigh_sigma is not None:
            ns = [float(v) for v in max_neigh_sigma.values()] if isinstance(max_neigh_sigma, dict) else [float(max_neigh_sigma)] * image.ndim
            neigh_sigma = tuple(s / float(sp) for s, sp in zip(ns, spacing))
    mask = detections(resp, window, threshold_abs, image, max_neigh_intensity, size, neigh_sigma)
    labels = ndimage.label(mask)[0].astype(np.int32)
    return (labels, resp, mask, threshold_abs) if return_parts else labels


def label_centroids(labels):
    """(n, ndim) float64 centres of mass of the labels of an integer label array, in label order (detect_beads'
    ``center_of_mass(labels, labels, ids)``)."""
    ids = np.unique(labels)
    ids = ids[ids > 0]
    if len(ids) == 0:
        return np.empty((0, labels.ndim), dtype=np.float64)
    return np.asarray(ndimage.center_of_mass(labels, labels=labels, index=ids), dtype=np.float64).reshape(len(ids), labels.ndim)


def runner_up_gaps(resp, mask, window):
    """For every detection: its response minus the largest value of any OTHER voxel in its (reflected) window; the voxel's own
    mirror images beyond a border do not count."""
    half = [w // 2 for w in window]
    pads = [(h, h) for h in half]
    padded = np.pad(resp, pads, mode="symmetric")
    source = np.pad(np.arange(resp.size).reshape(resp.shape), pads, mode="symmetric")
    gaps = []
    for idx in np.argwhere(mask):
        box = tuple(slice(int(i), int(i) + w) for i, w in zip(idx, window))
        others = padded[box][source[box] != np.ravel_multi_index(tuple(idx), resp.shape)]
        gaps.append(float(resp[tuple(idx)] - (others.max() if others.size else -np.inf)))
    return np.asarray(gaps)


def candidate_threshold_margin(resp, window, threshold):
    """min over the candidates (r == window maximum, r > 0) of |r - threshold| / threshold."""
    cand = (resp == ndimage.maximum_filter(resp, size=window, mode="reflect")) & (resp > 0)
    return float(np.min(np.abs(resp[cand] - threshold) / threshold)) if cand.any() else np.inf


def make_beads(shape, diameter, seed, dtype=np.uint16, n_beads=None, slab=None):
    """Seeded bead image: Gaussian blobs of sigma diameter / (2 sqrt(ndim)) (``diameter``: a number or one per axis, in voxels) at
    sub-voxel positions whose pairwise Chebyshev distance is at least 2.5 diameters, amplitudes uniform in [2000, 4000], on a
    background of 100 plus Gaussian noise of sigma 8; rounded and clipped to ``dtype`` (uint8: everything scaled by 1 / 20).  The
    first beads are placed within one radius of a border.  ``slab = (axis, lo, hi, level)`` adds a bright slab of that level
    whose faces are blurred (sigma 2 voxels, so that they raise no response of their own), for the neighbourhood-minimum rule.  Returns (image, positions (n, ndim) float64)."""
    rng = np.random.default_rng(seed)
    ndim = len(shape)
    diam = np.full(ndim, float(diameter)) if np.isscalar(diameter) else np.asarray(diameter, dtype=np.float64)
    sig = diam / (2.0 * np.sqrt(ndim))
    n = np.asarray(shape)
    if n_beads is None:
        n_beads = int(np.clip(np.prod(np.maximum(n / (3.5 * diam), 1.0)), 3, 40))
    pos = []
    for attempt in range(4000):
        if len(pos) >= n_beads:
            break
        p = rng.integers(0, n).astype(np.float64)
        if len(pos) < 2:                                   # a bead within one radius of a border
            ax = int(np.argmax(n / diam)) if len(pos) == 0 else int(rng.integers(0, ndim))
            p[ax] = float(rng.integers(0, max(int(diam[ax] / 2), 1))) if rng.random() < 0.5 else float(n[ax] - 1 - rng.integers(0, max(int(diam[ax] / 2), 1)))
        p += rng.uniform(-0.35, 0.35, ndim)
        if all(np.max(np.abs(p - q) / diam) >= 2.5 for q in pos):
            pos.append(p)
    pos = np.asarray(pos).reshape(-1, ndim)
    grids = np.meshgrid(*[np.arange(k, dtype=np.float64) for k in shape], indexing="ij")
    img = np.full(shape, 100.0)
    for p in pos:
        amp = rng.uniform(2000.0, 4000.0)
        img += amp * np.exp(-0.5 * sum(((g - c) / s) ** 2 for g, c, s in zip(grids, p, sig)))
    if slab is not None:
        ax, lo, hi, level = slab
        profile = np.zeros(shape[ax])
        profile[lo:hi] = level
        profile = ndimage.gaussian_filter1d(profile, 2.0, mode="nearest")
        img += profile.reshape([-1 if k == ax else 1 for k in range(ndim)])
    img += rng.normal(0.0, 8.0, shape)
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        img = img / 20.0
    if dtype.kind == "u":
        img = np.clip(np.rint(img), 0, np.iinfo(dtype).max)
    return img.astype(dtype), pos
