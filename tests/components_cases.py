"""Masks of the connected-component tests (tests/test_components_host.py, tests/test_components_gpu.py) at the smallest shapes that
reach every path: rows of 131 and 70 voxels have whole 64-voxel chunks, chunks off the 16-byte grid and tails; rows of 256 are all
whole and aligned.  Up to 8192 chunks every wave of the row launches takes one chunk; the shapes with more (``WIDE``) give a wave two
or more, so runs are carried from chunk to chunk and cut where one wave's range ends."""
import functools

import numpy as np

from tests import components_oracle as co


def _random(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def serpentine():
    """One path that fills 37 x 131: every other row whole, joined alternately at the right and the left end.  One component, and
    the longest chase a tile of this size can hold."""
    m = np.zeros((37, 131), dtype=bool)
    m[0::2] = True
    m[1::4, -1] = True
    m[3::4, 0] = True
    return m


def comb():
    """Teeth (every other column) that join only in the LAST row: 66 provisional roots collapse late."""
    m = np.zeros((37, 131), dtype=bool)
    m[:, 0::2] = True
    m[-1] = True
    return m


def nested_u():
    """Two U shapes, one inside the other, arms of unequal height.  In raster order the voxels (0, 40) outer right arm, (1, 10)
    inner left arm, (2, 30) inner right arm and (3, 0) outer left arm are met first: the outer U is 1 and the inner 2, while a
    numbering by provisional label or by the order the arms merge would differ.  A dot (5, 20) inside both is 3."""
    m = np.zeros((16, 50), dtype=bool)
    m[0:14, 40] = m[3:14, 0] = m[13, 0:41] = True      # outer
    m[1:10, 10] = m[2:10, 30] = m[9, 10:31] = True     # inner
    m[5, 20] = True
    return m


def checkerboard():
    """Every foreground voxel its own component at connectivity 1, one component at connectivity 2."""
    y, x = np.mgrid[:37, :131]
    return (y + x) % 2 == 0


def row_300():
    m = np.ones((1, 300), dtype=bool)
    m[0, [0, 63, 64, 130, 200, 201, 299]] = False      # runs that end on, begin on and cross the chunk boundaries
    return m


def aligned_256():
    m = _random((6, 256), 0.9, 31)
    m[2] = True
    m[3, :64] = True
    return m


def runs_across_ranges():
    """2100 x 300: 10 500 chunks, two per wave.  Even rows hold long runs (1 % gaps, a few rows whole) that cross chunks and the
    ends of the waves' ranges; odd rows are empty, so every run is a component and a run cut wrongly changes the count."""
    m = np.zeros((2100, 300), dtype=bool)
    m[0::2] = _random((1050, 300), 0.99, 32)
    m[0:40:2] = True
    return m


def all_foreground_wide():
    return np.ones((2100, 300), dtype=bool)


MASKS = {
    "random_2d_10": lambda: _random((37, 131), 0.10, 1),
    "random_2d_50": lambda: _random((37, 131), 0.50, 2),
    "random_2d_90": lambda: _random((37, 131), 0.90, 3),
    "random_3d_10": lambda: _random((5, 9, 70), 0.10, 4),
    "random_3d_50": lambda: _random((5, 9, 70), 0.50, 5),
    "random_3d_90": lambda: _random((5, 9, 70), 0.90, 6),
    "serpentine": serpentine,
    "comb": comb,
    "nested_u": nested_u,
    "checkerboard": checkerboard,
    "all_foreground": lambda: np.ones((37, 131), dtype=bool),
    "all_background": lambda: np.zeros((37, 131), dtype=bool),
    "single_voxel": lambda: np.ones((1, 1), dtype=bool),
    "row_300": row_300,
    "volume_5x1x9": lambda: _random((5, 1, 9), 0.6, 7),
    "aligned_256": aligned_256,
    "runs_across_ranges": runs_across_ranges,
    "all_foreground_wide": all_foreground_wide,
    "volume_40x70x131": lambda: _random((40, 70, 131), 0.35, 8),      # 8400 chunks: two per wave, and a scan of many blocks
}
WIDE = ("runs_across_ranges", "all_foreground_wide", "volume_40x70x131")
NAMES = sorted(MASKS)


@functools.lru_cache(maxsize=None)
def mask(name):
    m = MASKS[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def want(name, connectivity, min_voxels=1):
    """The oracle's ``(labels, n)`` of a mask; computed once and read-only."""
    labels, n = co.label_mask(mask(name), connectivity, min_voxels)
    labels.setflags(write=False)
    return labels, n


def connectivities(name):
    return list(range(1, mask(name).ndim + 1))


def as_image(m, dtype):
    """``(tile, threshold)``: the mask as an image tile of ``dtype`` whose background voxels EQUAL the threshold (uint16, float32);
    a uint8 mask goes with threshold 0."""
    if np.dtype(dtype) == np.uint8:
        return m.astype(np.uint8), 0.0
    if np.dtype(dtype) == np.uint16:
        return np.where(m, 40000, 300).astype(np.uint16), 300.0
    return np.where(m, 1.5, 0.25).astype(np.float32), 0.25


FLOAT_THRESHOLD = 0.5


@functools.lru_cache(maxsize=None)
def float_tile():
    """A float32 tile of 37 x 131 with NaNs, infinities and values equal to the threshold, all of them background but +inf."""
    rng = np.random.default_rng(9)
    t = rng.random((37, 131)).astype(np.float32)
    t[rng.random(t.shape) < 0.1] = np.nan
    t[rng.random(t.shape) < 0.1] = np.float32(FLOAT_THRESHOLD)
    t[rng.random(t.shape) < 0.02] = np.inf
    t[rng.random(t.shape) < 0.02] = -np.inf
    t[4, 60:70] = np.nextafter(np.float32(FLOAT_THRESHOLD), np.float32(1.0))      # the next float above: foreground
    t.setflags(write=False)
    return t


# ---- the disc mosaic as images ------------------------------------------------------------------------------------------------------
def disc_image_tiles():
    """``(truth mask, image sims)``: the disc mosaic of tests/labels_cases.py as uint16 image tiles -- discs 2000, background 100,
    cut at the same integer offsets -- to be thresholded at 1000 per tile."""
    from tests import labels_cases as lc

    truth = lc.disc_truth()
    image = np.where(truth > 0, 2000, 100).astype(np.uint16)
    sims = [lc.label_sim(np.ascontiguousarray(image[y0:y0 + lc.TILE_SHAPE[0], x0:x0 + lc.TILE_SHAPE[1]]), origin=(y0, x0)) for y0, x0 in lc.TILE_STARTS]
    return truth > 0, sims


DISC_THRESHOLD = 1000.0
