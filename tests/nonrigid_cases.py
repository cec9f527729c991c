"""Shared by tests/test_nonrigid_host.py and tests/test_nonrigid_gpu.py: the pair cases of the block-match tests (two tiles, blocks
with partial ones, a rotated moving map, halfspaces, part of the search window outside the moving tile) and the distorted mosaics of
the end-to-end tests with what the oracle alone makes of them -- built once."""
import functools

import numpy as np
from scipy import ndimage

from tests import nonrigid_oracle as no
from tests.intensity_helpers import DTYPES, rotation, texture
from tests.metrics_helpers import make_tile, translation_affine

MATCH = {3: dict(tile=(40, 48, 56), grid=(40, 48, 20), block=(12, 12, 12), radius=(2, 3, 3)),
         2: dict(tile=(96, 120), grid=(96, 45), block=(32, 32), radius=(6, 6))}


@functools.lru_cache(maxsize=None)
def match_case(ndim, dtype_name):
    """Two tiles cut from one scene so that the far ``grid`` columns of the fixed tile show the near ones of the moving tile; the
    moving map adds a rotation by 5 degrees about the grid centre and a fractional offset, the fixed map a fractional offset that
    puts the last plane / row of the grid outside the fixed tile; two halfspaces cut through blocks; the search window of the near
    blocks reaches outside the moving tile.  float32 tiles carry a few NaN voxels."""
    spec = MATCH[ndim]
    dtype = DTYPES[dtype_name]
    tile, grid = spec["tile"], spec["grid"]
    x0 = tile[-1] - grid[-1]
    scene = texture(tile[:-1] + (tile[-1] + x0,), 31 + ndim, dtype)
    fixed = np.ascontiguousarray(scene[..., :tile[-1]])
    moving = np.ascontiguousarray(scene[..., x0:])
    if dtype == np.float32:
        rng = np.random.default_rng(5)
        for t, xs in ((fixed, (x0 + 1, tile[-1] - 1)), (moving, (1, grid[-1]))):
            for _ in range(8):
                t[tuple(int(rng.integers(1, s - 1)) for s in tile[:-1]) + (int(rng.integers(*xs)),)] = np.nan
    fixed_affine = (np.eye(ndim), np.array([0.3137, 0.2713, x0 - 0.5481][-ndim:]))
    gctr = (np.asarray(grid, dtype=float) - 1) / 2
    rot = rotation(ndim, np.deg2rad(5.0))
    target = gctr + np.array([0.1731, 0.6177, 0.7893][-ndim:])
    moving_affine = (rot, target - rot @ gctr)
    rows = []
    for sign, angle, frac in ((1, 0.35, 0.31), (-1, -0.2, 0.36)):
        n2 = sign * rotation(2, angle)[0]
        n = np.concatenate([np.zeros(ndim - 2), n2])
        rows.append(np.concatenate([n, [-(n @ gctr) - frac * grid[-2] - 0.0137]]))
    blocks = no.plan_blocks(grid, spec["block"], fixed_affine, moving_affine, tile, tile, (2,) * ndim, (2,) * ndim)[:, :2]
    return {"fixed": fixed, "moving": moving, "grid_shape": grid, "fixed_affine": fixed_affine, "moving_affine": moving_affine,
            "halfspaces": np.array(rows), "blocks": blocks, "radius": spec["radius"]}


@functools.lru_cache(maxsize=None)
def match_oracle(ndim, dtype_name):
    c = match_case(ndim, dtype_name)
    return no.block_moments(c["fixed"], c["moving"], c["fixed_affine"], c["moving_affine"], c["blocks"], c["radius"], c["halfspaces"])


def largest_block(grid, limit=7680):
    """``(1, 2, ndim)`` blocks with the largest box at ``lo = 0`` of ``grid`` that has at most ``limit`` points (of equally large ones
    the one with the longest rows, then planes).  7680: at radius 0 the grown block is the block, and mvs_block_match keeps both
    (MVS_BLOCKMATCH_MAX_FLOATS = 15 360 samples)."""
    shapes = np.stack(np.meshgrid(*[np.arange(1, g + 1) for g in grid], indexing="ij"), axis=-1).reshape(-1, len(grid))
    shapes = shapes[shapes.prod(axis=1) <= limit]
    n = max(shapes.tolist(), key=lambda s: (int(np.prod(s)),) + tuple(s[::-1]))
    return np.array([[[0] * len(grid), n]], dtype=np.int64)


# ---- the distorted mosaics ------------------------------------------------------------------------------------------------------
# per case: the mosaic's ndim and the arguments of fit_fields; "2d_tight" has a window that is too small for some blocks (rim) and a
# threshold that some peaks miss (low_ncc)
FIT = {"2d": dict(ndim=2, nodes=(4, 4), block=(32, 32), radius=(6, 6), min_ncc=0.3),
       "3d": dict(ndim=3, nodes=(2, 2, 2), block=(12, 12, 12), radius=(3, 3, 3), min_ncc=0.3),
       "2d_tight": dict(ndim=2, nodes=(3, 2), block=(32, 24), radius=(1, 1), min_ncc=0.982)}
LAMBDAS = dict(lambda_identity=0.05, lambda_smooth=0.1)


def distortion(shape, seed, amplitude):
    """A smooth displacement (ndim, *shape) of at most ``amplitude`` px per component: one low-frequency wave per component."""
    rng = np.random.default_rng(seed)
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) / n for n in shape], indexing="ij")
    out = []
    for _ in shape:
        phase = rng.uniform(0, 2 * np.pi, len(shape))
        freq = rng.uniform(0.6, 1.4, len(shape))
        out.append(amplitude * np.prod([np.sin(np.pi * f * i + p) for f, i, p in zip(freq, idx, phase)], axis=0))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def mosaic(ndim):
    """2D: a 2 x 2 mosaic of 160 x 160 float32 tiles that overlap by 48 px; 3D: two 48 x 64 x 64 uint16 tiles that overlap by 24 px
    along x.  The tiles are cut from one smoothed-noise texture, tile v showing G(origin_v + p + e_v(p)) with a smooth distortion
    e_v of its own of at most 1.5 px.  Returns msims, oracle views, pairs and the distortions."""
    if ndim == 2:
        tile, origins, dtype, comp = (160, 160), [(0, 0), (0, 112), (112, 0), (112, 112)], np.float32, 1.0
    else:
        tile, origins, dtype, comp = (48, 64, 64), [(0, 0, 0), (0, 0, 40)], np.uint16, 0.85
    pad = 4
    full = tuple(max(o[k] for o in origins) + tile[k] + 2 * pad for k in range(ndim))
    rng = np.random.default_rng(40 + ndim)
    g = ndimage.gaussian_filter(rng.standard_normal(full), 2.0)
    g = (g - g.min()) / (g.max() - g.min())
    msims, views, fields = [], [], []
    for v, o in enumerate(origins):
        e = distortion(tile, 50 + 10 * ndim + v, comp)
        assert np.sqrt((e ** 2).sum(axis=0)).max() <= 1.5
        idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in tile], indexing="ij")
        cut = ndimage.map_coordinates(g, [i + o[k] + pad + e[k] for k, i in enumerate(idx)], order=3, mode="nearest")
        data = (cut * 3.0 + 0.5).astype(np.float32) if dtype == np.float32 else np.rint(cut * 60000.0).astype(np.uint16)
        m, view = make_tile(data, {"stage": translation_affine([float(x) for x in o])})
        msims.append(m)
        views.append(view)
        fields.append(e)
    pairs = [(i, j) for i in range(len(origins)) for j in range(i + 1, len(origins))
             if all(abs(a - b) < t for a, b, t in zip(origins[i], origins[j], tile)) and sum(a != b for a, b in zip(origins[i], origins[j])) == 1]
    return {"msims": msims, "views": views, "pairs": pairs, "distortions": fields, "tile": tile, "origins": origins}


@functools.lru_cache(maxsize=None)
def oracle_fit(name):
    """(fields, info) of the oracle on the mosaic of case ``name``."""
    f = FIT[name]
    m = mosaic(f["ndim"])
    return no.fit_fields(m["views"], "stage", f["nodes"], m["pairs"], f["block"], f["radius"], min_ncc=f["min_ncc"], **LAMBDAS)


@functools.lru_cache(maxsize=None)
def oracle_ratio(name):
    """The weighted RMS shift that block matching finds on the tiles the oracle corrected, over the one on the given tiles."""
    f = FIT[name]
    m = mosaic(f["ndim"])
    fields, info = oracle_fit(name)
    corrected = [dict(v, data=no.warp(v["data"], d)) for v, d in zip(m["views"], fields)]
    _, records = no.match_pairs(corrected, "stage", f["nodes"], m["pairs"], f["block"], f["radius"], min_ncc=f["min_ncc"])
    return no.rms(records) / info["rms_before"]


def assert_margins(info, min_samples=64, min_ncc=0.3, min_kept=4):
    """The oracle alone leaves margins that 1e-9 of NCC noise cannot flip: every kept block's peak leads its runner-up by at least
    1e-6, every threshold is cleared or missed by at least 1e-6 relative, every examined second difference is at most -1e-2."""
    kept = 0
    for blocks, found in info["per_pair"].values():
        for f in found:
            assert abs(f["n"] - min_samples) >= 1e-6 * min_samples
            if f["reason"] == "few_samples":
                continue
            assert not np.isnan(f["peak"]) and abs(f["peak"] - min_ncc) >= 1e-6 * min_ncc
            if f["reason"] == "low_ncc":
                continue
            assert f["peak"] - f["runner_up"] >= 1e-6, f          # (also for the blocks dropped for a peak on the rim)
            if f["reason"] is None:
                kept += 1
                assert max(f["second"]) <= -1e-2, f
            else:
                assert f["reason"] == "rim", f                  # no block of these inputs is flat
    assert kept >= min_kept
    return kept
