"""Seeded inputs of the multi-band fusion tests, shared by the host tests (conditioning of every input) and the GPU tests (the same
inputs against the oracle).  Intensities stay near 100 +- 10, well away from 0, so the float bar is a relative one everywhere."""
import functools

import numpy as np

# the REDUCE tile of csrc/mvs_multiband_plan.h in level-l samples: a workgroup step reads 32 x 64 (y, x) samples (+ apron) of one plane
REDUCE_TILE = (32, 64)


def make_views(shape, n_views, seed, gains=None, full=False):
    """(V, B) float32 of shape (n_views, *shape): smooth content around 100 with per-view gain, offset and noise; every view covers a
    box of its own with a ragged lower edge along the last axis (NaN outside), the boxes overlap in the middle and touch the array's
    borders, and one band of rows is covered by no view.  B: raw ramp weights >= 0, also where the view is NaN.  ``full``: every view
    is finite everywhere (the views disagree everywhere), the weights stay the ramps of the boxes."""
    rng = np.random.default_rng(seed)
    ndim = len(shape)
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    base = 100.0 + 6.0 * np.sin(0.31 * grids[-1] + 0.2) * np.cos(0.23 * grids[-2] if ndim > 1 else 0.0) + 3.0 * np.sin(0.11 * sum(grids))
    V, B = [], []
    for v in range(n_views):
        gain = (1.0 + 0.04 * ((v % 3) - 1)) if gains is None else gains[v]
        img = base * gain + (v - n_views / 2) * 0.7 + rng.normal(0.0, 1.5, shape)
        lo, hi = [], []
        for d, n in enumerate(shape):
            if n < 8 or d < ndim - 2:          # short axes and z: covered whole
                lo.append(0), hi.append(n)
                continue
            span = max(4, int(round(n * 0.62)))
            a = int(round((n - span) * (v / max(1, n_views - 1)))) if n_views > 1 else 0
            lo.append(a), hi.append(min(n, a + span))
        idx = np.ogrid[tuple(slice(0, n) for n in shape)]
        inside = np.ones(shape, bool)
        w = np.ones(shape, np.float64)
        for d in range(ndim):
            inside &= (idx[d] >= lo[d]) & (idx[d] < hi[d])
            width = max(1.0, min(10.0, (hi[d] - lo[d]) / 2))
            w = w * np.clip(np.minimum(idx[d] - lo[d] + 1, hi[d] - idx[d]) / width, 0.0, 1.0)
        if ndim > 1 and shape[-1] >= 8:          # ragged lower edge along x, row by row
            ragged = (np.arange(shape[-2]) * 7 + v * 3) % 4
            inside &= idx[-1] >= (lo[-1] + ragged).reshape((-1, 1))
        if ndim > 1 and shape[-2] >= 24:         # a band no view covers
            inside &= ~((idx[-2] >= shape[-2] // 3) & (idx[-2] < shape[-2] // 3 + 2))
        V.append(img if full else np.where(inside, img, np.nan))
        B.append(w + 0.01 * rng.random(shape))
    return np.stack(V).astype(np.float32), np.stack(B).astype(np.float32)


@functools.lru_cache(maxsize=None)
def float_cases():
    """name -> (V, B, n_levels, index_origin); built once, read-only for every test."""
    ty, tx = REDUCE_TILE
    cases = {
        "2d_L3": make_views((70, 90), 2, 1) + (3, None),
        "3d_levels_122": make_views((6, 40, 44), 3, 2) + ({"z": 1, "y": 2, "x": 2}, None),
        "origin_-12_23": make_views((37, 41), 2, 3) + (2, (-12, 23)),
        "origin_1_1": make_views((37, 41), 2, 4) + (2, (1, 1)),
        "length_1": make_views((1, 40), 2, 5) + (2, None),
        "length_2": make_views((2, 40), 2, 6) + (2, None),
        "tile_plus_1": make_views((ty + 1, tx + 1), 2, 7) + (2, None),
        "tile_minus_1": make_views((ty - 1, tx - 1), 2, 8) + (2, None),
        "tile_z_3d": make_views((5, ty + 1, tx - 1), 2, 9) + (1, (3, -1, 2)),
        "views_1": make_views((30, 34), 1, 10) + (2, None),
        "views_9": make_views((30, 34), 9, 11) + (2, None),
        "levels_0": make_views((40, 50), 2, 12) + (0, None),
        "levels_6": make_views((70, 90), 2, 13) + (6, None),
        # past the first trip of every capped grid-stride launch (2048 workgroups): 2.25 M voxels = 2198 workgroups of prepare, 4512
        # REDUCE steps and 2209 workgroups of the level-1 collapse
        "grid_stride": make_views((1500, 1500), 2, 14) + (2, (5, -3)),
    }
    for V, B, _, _ in cases.values():
        V.setflags(write=False), B.setflags(write=False)
    return cases


# The cap on u8 voxels that may differ by one count between two float evaluations of one input: a voxel can only differ when its float
# value is within the float bar of a rounding boundary k + 0.5; the bar is at most 1e-4 * 255 = 0.0255 counts on either side of the
# boundary, i.e. a share of 2 * 0.0255 = 5.1 % of values spread evenly over a count.
U8_DIFFER_CAP = 2 * 1e-4 * 255


def checker_u8():
    """(V uint8, B float32, n_levels): two views holding opposite 0 / 255 checker patterns over the whole 48 x 64 array, smooth random
    ramp weights: the bands overshoot 0 and 255."""
    rng = np.random.default_rng(21)
    shape = (48, 64)
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    checker = (((yy // 3) + (xx // 3)) % 2).astype(np.uint8) * 255
    V = np.stack([checker, 255 - checker]).astype(np.uint8)
    ramp = (xx + 0.37) / shape[1]
    B = np.stack([1.0 - 0.83 * ramp, 0.11 + 0.89 * ramp]) + 0.05 * rng.random((2,) + shape)
    return V, B.astype(np.float32), 2


def float_bar(want, rtol=1e-4):
    """The project's float bar (tests.helpers.fused_close_stats) per voxel: rtol * max(|want|, 1e-3 * range)."""
    rng = float(np.nanmax(np.abs(want)) or 1.0)
    return rtol * np.maximum(np.abs(want), 1e-3 * rng)
