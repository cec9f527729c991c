"""numpy / scipy restatement of the sample-mask kernels (csrc/mvs_masks.hip), written from their stated semantics:
``np.histogram`` for the counts, ``scipy.ndimage.maximum_filter`` for the dilation, ``oracle.fuse_oracle.transform_array`` at
order 0 with NaN outside, ``nanmin`` and ``nan_to_num`` for the label fuse, and one shifted-slice comparison per offset of the half
neighbourhood for the contacts."""
import itertools
import warnings

import numpy as np
from scipy import ndimage

from multiview_stitcher_amd import spatial_image_utils as si
from oracle import fuse_oracle as fo


def value_range(tiles):
    values = np.concatenate([np.asarray(t, dtype=np.float64).ravel() for t in tiles])
    valid = values[~np.isnan(values)]
    return float(valid.min()), float(valid.max()), int(valid.size)


def histogram(tiles, n_bins, lo, hi):
    values = np.concatenate([np.asarray(t).ravel() for t in tiles]).astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (NaNs compare false against the range)
        counts, edges = np.histogram(values, bins=n_bins, range=(lo, hi))
    return counts.astype(np.uint64), edges


def threshold_mask(tile, threshold, radius):
    tile = np.asarray(tile)
    if tile.dtype == np.float32:
        mask = tile > np.float32(threshold)
    else:
        mask = tile.astype(np.float64) > float(threshold)
    mask = mask.astype(np.uint8)
    if any(radius):
        mask = ndimage.maximum_filter(mask, size=[2 * r + 1 for r in radius], mode="constant", cval=0)
    return mask


def fuse_labels(masks, params, origins, spacings, out_bb):
    """nan_to_num(nanmin_i transform(mask_i * (i + 1), order 0, NaN outside)) as int32; ``params``: view -> world affines."""
    stack = [fo.transform_array((np.asarray(m) != 0).astype(np.float32) * (i + 1), np.linalg.inv(p), o, s, out_bb, order=0, cval=np.nan)
             for i, (m, p, o, s) in enumerate(zip(masks, params, origins, spacings))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (all-NaN voxels: no view covers them)
        fused = np.nanmin(np.stack(stack), axis=0)
    return np.nan_to_num(fused).astype(np.int32)


def sampling_coordinates(param, origin, spacing, out_bb):
    """The coordinates (ndim, *out_shape) at which the label fuse samples a view, in pixels of the view."""
    matrix, offset = fo.transform_params(np.linalg.inv(param), origin, spacing, out_bb)
    grid = np.stack(np.meshgrid(*[np.arange(int(n), dtype=np.float64) for n in out_bb["shape"]], indexing="ij"))
    return np.tensordot(matrix, grid, axes=1) + offset.reshape((-1,) + (1,) * (grid.ndim - 1))


def half_neighbourhood(ndim, connectivity):
    """Of every offset in {-1, 0, 1}^ndim with 1 .. connectivity non-zero components and its negative, the one whose first
    non-zero component is +1."""
    out = []
    for o in itertools.product((-1, 0, 1), repeat=ndim):
        nonzero = [v for v in o if v]
        if 1 <= len(nonzero) <= connectivity and nonzero[0] > 0:
            out.append(o)
    return out


def contact_counts(labels, n_labels, connectivity=None):
    labels = np.asarray(labels)
    ndim = labels.ndim
    connectivity = ndim if connectivity is None else connectivity
    counts = np.zeros((n_labels, n_labels), dtype=np.uint64)
    for o in half_neighbourhood(ndim, connectivity):
        here = tuple(slice(max(-d, 0), n - max(d, 0)) for d, n in zip(o, labels.shape))
        there = tuple(slice(max(d, 0), n - max(-d, 0)) for d, n in zip(o, labels.shape))
        a, b = labels[here].ravel(), labels[there].ravel()
        keep = (a > 0) & (b > 0) & (a != b)
        lo, hi = np.minimum(a[keep], b[keep]) - 1, np.maximum(a[keep], b[keep]) - 1
        np.add.at(counts, (lo, hi), np.uint64(1))
    return counts


def pairs_of(counts):
    return [(int(i), int(j)) for i, j in zip(*np.nonzero(np.triu(counts, 1)))]


# ---- a case the GPU tests and smoke() share ------------------------------------------------------------------------------------------
def sparse_row(key):
    """Four tiles of 64 x 64 in a row, 16 voxels of overlap: sample in the tiles 0 and 1 (one piece across their overlap) and in
    tile 3; tile 2 is empty and separates them."""
    rng = np.random.default_rng(21)
    scene = np.full((64, 208), 100.0)        # (Otsu's threshold is a bin centre: a background of one value ends below it)
    texture = rng.integers(600, 1400, (64, 208)).astype(np.float64)
    scene[12:50, 20:91] = texture[12:50, 20:91]
    scene[20:40, 170:191] = texture[20:40, 170:191]
    sims = []
    for i in range(4):
        x0 = 48 * i
        sim = si.to_spatial_image(np.ascontiguousarray(scene[:, x0:x0 + 64]).astype(np.uint16), dims=["y", "x"], scale={"y": 1.0, "x": 1.0},
                                  translation={"y": 0.0, "x": float(x0)})
        si.set_sim_affine(sim, np.eye(3), key)
        sims.append(sim)
    return sims, scene
