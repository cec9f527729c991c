"""Masks of the feather tests (tests/test_mask_feather_host.py, tests/test_mask_feather_gpu.py, the weight tiles of
tests/test_fuse_weighted_gpu.py): smooth random blobs with 35 % background, and the (shape, widths) table the kernel is held to.

  the first five   the shapes and widths the integer scheme was checked on against scipy: a wide y / x window on a thin stack, width 1
                   along an axis of one voxel, a row longer than two 64-bit windows, 2-D, and width 32 on a mask far smaller than it
  window_over_axis every window exceeds its axis
  x64 / x65 / x127 row lengths at the edges of the x pass's groups of 16 voxels and of its 80-bit window, width 8
  2-D              one more plane mask, with unequal widths
"""
import functools

import numpy as np
from scipy import ndimage

CASES = {
    "thin_stack": ((12, 20, 37), (2, 8, 8)),
    "one_plane_w32": ((1, 33, 70), (1, 32, 32)),
    "long_rows": ((5, 9, 130), (3, 3, 5)),
    "plane_40x67": ((40, 67), (6, 11)),
    "tiny_w32": ((3, 4, 5), (32, 32, 32)),
    "window_over_axis": ((7, 5, 3), (32, 32, 32)),
    "x64": ((3, 6, 64), (2, 3, 8)),
    "x65": ((3, 6, 65), (2, 3, 8)),
    "x127": ((2, 5, 127), (2, 3, 8)),
    "plane_33x50": ((33, 50), (4, 17)),
}


@functools.lru_cache(maxsize=None)
def blob_mask(shape, seed=7, background=0.35, sigma=2.0):
    """uint8 0 / 1: a smoothed random field above its ``background`` quantile.  Built once per argument set; leave it unchanged."""
    field = ndimage.gaussian_filter(np.random.default_rng(seed).random(shape), sigma, mode="nearest")
    mask = (field > np.quantile(field, background)).astype(np.uint8)
    mask.setflags(write=False)
    return mask


def first_plane_last_column(shape):
    """A mask whose zeros lie only in the first plane and the last column."""
    mask = np.ones(shape, np.uint8)
    mask[0] = 0
    mask[..., -1] = 0
    return mask
