"""Shared by tests/test_intensity_host.py and tests/test_intensity_gpu.py: the pair cases (two tiles, a grid, a rotated moving
map, halfspaces) and the mosaics of the end-to-end tests, built once."""
import functools

import numpy as np
from scipy import ndimage

from tests.metrics_helpers import make_tile, translation_affine

DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
TILE = {2: (40, 52), 3: (12, 20, 36)}
CELLS = {2: ((2, 3), (3, 2)), 3: ((1, 2, 3), (2, 1, 2))}


def texture(shape, seed, dtype):
    rng = np.random.default_rng(seed)
    t = ndimage.gaussian_filter(rng.random(shape), 1.2)
    t = (t - t.min()) / (t.max() - t.min())
    if dtype == np.uint8:
        return (t * 255).astype(np.uint8)
    if dtype == np.uint16:
        return (t * 60000).astype(np.uint16)
    return (t * 3.0 + 0.5).astype(np.float32)


def rotation(ndim, angle):
    m = np.eye(ndim)
    c, s = np.cos(angle), np.sin(angle)
    m[-2:, -2:] = [[c, -s], [s, c]]
    return m


@functools.lru_cache(maxsize=None)
def pair_case(ndim, dtype_name, step=1):
    """Two tiles of TILE[ndim] cut from one scene, a grid of the tile's extent sampled every ``step`` pixels, the moving tile under a
    sub-pixel shift plus a rotation by 5 degrees about the centre, and a rotated box of halfspaces that cuts through the grid."""
    dtype = DTYPES[dtype_name]
    shape = TILE[ndim]
    scene = texture(tuple(s + 8 for s in shape), 21 + ndim, dtype)
    fixed = np.ascontiguousarray(scene[tuple(slice(2, 2 + s) for s in shape)])
    moving = np.ascontiguousarray(scene[tuple(slice(4, 4 + s) for s in shape)])
    grid_shape = tuple((s - 1) // step + 1 for s in shape)
    fixed_affine = (np.eye(ndim) * float(step), np.array([0.3137, 0.2713, 0.4519][-ndim:]))
    ctr = (np.asarray(shape, dtype=float) - 1) / 2
    rot = rotation(ndim, np.deg2rad(5.0))
    shift = np.array([0.1731, -1.6177, 2.2893][-ndim:])
    moving_affine = (rot * float(step), ctr - rot @ ctr + shift + rot @ fixed_affine[1])
    gctr = (np.asarray(grid_shape, dtype=float) - 1) / 2
    half = 0.46 * np.asarray(grid_shape[-2:], dtype=float)
    rows = []
    for ax, sign in ((0, 1), (0, -1), (1, 1), (1, -1)):
        n2 = sign * rotation(2, 0.35)[ax]
        n = np.concatenate([np.zeros(ndim - 2), n2])
        rows.append(np.concatenate([n, [-(n @ gctr) - half[ax] - 0.0137]]))
    return {"fixed": fixed, "moving": moving, "grid_shape": grid_shape, "fixed_affine": fixed_affine, "moving_affine": moving_affine,
            "halfspaces": np.array(rows), "cells_f": CELLS[ndim][0], "cells_m": CELLS[ndim][1]}


def smooth_field(shape, seed):
    """A smooth positive random field with values around 1."""
    rng = np.random.default_rng(seed)
    t = ndimage.gaussian_filter(rng.random(shape), 3.0)
    return ((t - t.min()) / (t.max() - t.min()) + 0.5).astype(np.float64)


@functools.lru_cache(maxsize=None)
def mosaic(ndim, ramp=False):
    """Float32 tiles cut from one smooth field at integer offsets with 16-pixel overlaps: 2 x 2 tiles of 64 x 64, or 2 x 1 x 2 tiles
    of 16 x 48 x 48.  Tile v is stored as ``g_v * field + o_v`` (``ramp``: the gain also rises by 10 % across the tile along x).
    Returns msims, oracle views, clean msims (no gains), the gains and offsets, and the pairs."""
    if ndim == 2:
        tile, grid, ov = (64, 64), (2, 2), 16
    else:
        tile, grid, ov = (16, 48, 48), (2, 1, 2), 16
    steps = [t - ov for t in tile]
    if ndim == 3:
        steps[0] = tile[0] - 8
    full = tuple(s * (g - 1) + t for s, g, t in zip(steps, grid, tile))
    field = smooth_field(full, 3 + ndim)
    gains = [1.0, 1.25, 0.8, 1.1]
    offsets = [0.0, 0.05, -0.03, 0.02]
    msims, views, clean = [], [], []
    origins = []
    for v, pos in enumerate(np.ndindex(*grid)):
        o = [p * s for p, s in zip(pos, steps)]
        origins.append(o)
        cut = field[tuple(slice(a, a + t) for a, t in zip(o, tile))]
        g = gains[v] * (1.0 + 0.1 * np.linspace(-0.5, 0.5, tile[-1])) if ramp else gains[v]
        data = (g * cut + offsets[v]).astype(np.float32)
        aff = {"stage": translation_affine([float(x) for x in o])}
        m, view = make_tile(data, aff)
        msims.append(m)
        views.append(view)
        clean.append(make_tile(cut.astype(np.float32), aff)[0])
    pairs = []
    for i in range(len(origins)):
        for j in range(i + 1, len(origins)):
            if all(abs(a - b) < t for a, b, t in zip(origins[i], origins[j], tile)):
                pairs.append((i, j))
    return {"msims": msims, "views": views, "clean": clean, "gains": gains, "offsets": offsets, "pairs": pairs, "tile": tile, "origins": origins}
