"""The restatement of labels.label_components / mvs_label_components: scipy.ndimage.label on the thresholded tile, small components
dropped and the rest renumbered in order."""
import numpy as np
from scipy import ndimage


def foreground(tile, threshold):
    """The foreground rule: ``(float32)v > (float32)threshold`` -- a voxel equal to the threshold and a NaN are background."""
    with np.errstate(invalid="ignore"):
        return np.asarray(tile).astype(np.float32) > np.float32(threshold)


def label_mask(mask, connectivity=1, min_voxels=1):
    """``(labels int32, n)`` of a boolean mask: scipy.ndimage.label with generate_binary_structure(ndim, connectivity); the
    components with fewer than ``min_voxels`` voxels become 0 and the others are renumbered 1 .. n in their order."""
    mask = np.asarray(mask, dtype=bool)
    labels, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(mask.ndim, connectivity))
    labels = labels.astype(np.int32)
    if min_voxels > 1 and n:
        keep = np.bincount(labels.ravel(), minlength=n + 1) >= min_voxels
        keep[0] = False
        lut = np.zeros(n + 1, dtype=np.int32)
        lut[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
        labels, n = lut[labels], int(keep.sum())
    return labels, int(n)


def label_components(tile, threshold, connectivity=1, min_voxels=1):
    return label_mask(foreground(tile, threshold), connectivity, min_voxels)
