"""Inputs of the label-stitching tests (tests/test_labels_host.py, tests/test_labels_gpu.py): label sims with a transform, the pixel
affines the oracle (tests/labels_oracle.py) takes for them, and a mosaic of discs cut into overlapping tiles."""
import numpy as np

from multiview_stitcher_amd import fusion
from multiview_stitcher_amd import spatial_image_utils as si
from tests import labels_oracle as lo

KEY = "stage"


def label_sim(tile, origin=None, affine=None, spacing=None):
    """A 2-D / 3-D label sim: ``tile`` (a numpy array or a DeviceArray) at ``origin`` with ``spacing`` and ``affine`` under KEY."""
    ndim = len(tile.shape)
    sdims = ["z", "y", "x"][3 - ndim:]
    origin = [0.0] * ndim if origin is None else origin
    spacing = [1.0] * ndim if spacing is None else spacing
    sim = si.to_spatial_image(tile, dims=sdims, scale=dict(zip(sdims, map(float, spacing))), translation=dict(zip(sdims, map(float, origin))))
    si.set_sim_affine(sim, np.eye(ndim + 1) if affine is None else np.asarray(affine, dtype=np.float64), KEY)
    return sim


def rotation(ndim, degrees, centre, shift=None):
    """The affine that turns by ``degrees`` in the (y, x) plane about ``centre`` and then shifts."""
    t = np.deg2rad(degrees)
    R = np.eye(ndim)
    R[-2:, -2:] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
    centre = np.asarray(centre, dtype=np.float64)
    A = np.eye(ndim + 1)
    A[:ndim, :ndim] = R
    A[:ndim, ndim] = centre - R @ centre + (0.0 if shift is None else np.asarray(shift, dtype=np.float64))
    return A


def _geometry(sim):
    return (np.asarray(si.get_affine_from_sim(sim, KEY), dtype=np.float64), si.get_origin_from_sim(sim, asarray=True),
            si.get_spacing_from_sim(sim, asarray=True))


def pair_affine(sim_a, sim_b):
    """(matrix, offset) from a pixel index of ``a`` to a pixel coordinate of ``b``, by the oracle's own derivation."""
    (Ta, Oa, Sa), (Tb, Ob, Sb) = _geometry(sim_a), _geometry(sim_b)
    return lo.pixel_affine(np.linalg.inv(Tb) @ Ta, Ob, Sb, Oa, Sa)


def oracle_pair_table(sim_a, sim_b):
    return lo.pair_table(np.asarray(sim_a.data), np.asarray(sim_b.data), *pair_affine(sim_a, sim_b))


def whole_grid(sims, spacing=None):
    """The grid of ``fusion.calc_fusion_stack_properties`` of the sims (the definition of the fused image's grid)."""
    sdims = si.get_spatial_dims_from_sim(sims[0])
    spacing = si.get_spacing_from_sim(sims[0]) if spacing is None else dict(zip(sdims, spacing))
    return fusion.calc_fusion_stack_properties(sims, [_geometry(s)[0] for s in sims], spacing, mode="union")


def oracle_fuse(sims, luts=None, grid=None, box=None):
    """The oracle's fused image of the sims on ``grid`` (default: the whole grid); ``box`` = (first index, shape) of a part of it."""
    sdims = si.get_spatial_dims_from_sim(sims[0])
    grid = whole_grid(sims) if grid is None else grid
    O, S = np.array([grid["origin"][d] for d in sdims]), np.array([grid["spacing"][d] for d in sdims])
    affines = [lo.pixel_affine(np.linalg.inv(T), Ov, Sv, O, S) for T, Ov, Sv in map(_geometry, sims)]
    origin, shape = ([0] * len(sdims), [int(grid["shape"][d]) for d in sdims]) if box is None else box
    return lo.fuse([np.asarray(s.data) for s in sims], [m for m, _ in affines], [o for _, o in affines], luts, tuple(shape), origin)


def sub_grid(grid, first, shape):
    """The stack properties of the box of ``grid`` that starts at the index ``first``."""
    sdims = list(grid["shape"])
    return {"shape": dict(zip(sdims, map(int, shape))), "spacing": dict(grid["spacing"]),
            "origin": {d: grid["origin"][d] + f * grid["spacing"][d] for d, f in zip(sdims, first)}}


# ---- the disc mosaic ----------------------------------------------------------------------------------------------------------------
TRUTH_SHAPE = (96, 150)
TILE_SHAPE = (56, 85)
TILE_STARTS = [(0, 0), (0, 65), (40, 0), (40, 65)]      # 2 x 2 tiles: 16 rows and 20 columns of overlap
N_DISCS = 82


def disc_truth(seed=5):
    """A (96, 150) int32 image of 82 discs with the ids 1 .. 82 that do not touch: one disc per cell of a 7 x 12 grid (two cells left
    empty), radius 3 .. 4.5, centre within one pixel of the cell's."""
    rng = np.random.default_rng(seed)
    truth = np.zeros(TRUTH_SHAPE, dtype=np.int32)
    yy, xx = np.mgrid[:TRUTH_SHAPE[0], :TRUTH_SHAPE[1]]
    cells = [(i, j) for i in range(7) for j in range(12)]
    keep = sorted(rng.choice(len(cells), N_DISCS, replace=False))
    for label, k in enumerate(keep, start=1):
        i, j = cells[k]
        cy = (i + 0.5) * TRUTH_SHAPE[0] / 7 + rng.uniform(-1, 1)
        cx = (j + 0.5) * TRUTH_SHAPE[1] / 12 + rng.uniform(-1, 1)
        r = rng.uniform(3.0, 4.5)
        truth[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = label
    return truth


def disc_mosaic(seed=5):
    """``(truth, tiles, sims)``: the disc image cut into the 2 x 2 tiles at integer offsets, every tile with a random relabelling of
    its own into distinct ids of 1 .. 199 999 -- half of them above 65 535 -- as int32 label sims at the tiles' origins."""
    rng = np.random.default_rng(seed + 1)
    truth = disc_truth(seed)
    tiles = []
    for y0, x0 in TILE_STARTS:
        new = np.zeros(N_DISCS + 1, dtype=np.int32)
        new[1:] = np.concatenate([rng.choice(np.arange(1, 65536), N_DISCS // 2, replace=False),
                                  rng.choice(np.arange(65536, 200000), N_DISCS - N_DISCS // 2, replace=False)])[rng.permutation(N_DISCS)]
        tiles.append(np.ascontiguousarray(new[truth[y0:y0 + TILE_SHAPE[0], x0:x0 + TILE_SHAPE[1]]]))
    return truth, tiles, [label_sim(t, origin=o) for t, o in zip(tiles, TILE_STARTS)]
