"""Case table of the generic affine fuse kernel's tests (tests/test_affine_cases_host.py, tests/test_fuse_generic_gpu.py): chunks whose
views carry a matrix that is not the identity -- rotations through large angles, permutations and mirrors, shear with anisotropic
spacings -- built on the CPU from ``helpers.white_noise`` tiles (two views differ by a third of the range at a voxel, so a wrong weight
or a dropped view moves the output by whole counts).  A case is ``(sims, params, out_bb, kwargs)``: squeezed sims, one view -> world
matrix per view, the chunk's box in the oracle's data model, and what ``helpers.run_both`` takes besides (the trim).  The host test
checks with the oracle alone that every case is what it says it is; the GPU test runs the library on it.

  fan3d_12, fan2d_12   12 views turned about the tile centre by 360 * i / 12 degrees, each moved by a fractional shift of +-2: more than
                       8 views on a brick (the 9th and later read their blend table from global memory) and large angles in the cull
  fan2d_70             70 views turned by 360 * i / 70 degrees: both cull batches (base = 0 and 64) with real matrices
  knife_rot90 (2D, 3D) identity, np.pi / 2 and np.pi about the tile centre; borders on integer output voxels, coordinates within 1e-9 of
                       0 and n - 1 on either side of them (see ``_knife_rot90``)
  mirror_swap          exact permutation and sign matrices, integer offsets: coordinates equal to 0.0 and n - 1; float32 tiles carry NaNs
                       at n - 2 (the mirrored second tap of n - 1) and at random voxels
  mirror_swap_one_rotated   the same tiles under integer translations, the last view turned by 30 degrees: routing only
  shear_aniso          shear, +-10 % scale, one negative determinant, input spacing (2.0, 0.8, 1.3) onto (1.0, 0.75, 1.25); the third view
                       reaches the chunk with a corner only
  trimmed              shear_aniso under trim_overlap_in_pixels = 3: a result width that is no multiple of 4
  far_origin           two turned views whose world origins lie near 1e5
"""
import functools

import numpy as np

from oracle import fuse_oracle as fo
from tests.helpers import sim_to_view, squeeze_field, union_bb, white_noise

SDIMS = ["z", "y", "x"]
NAMES = ("fan3d_12", "fan2d_12", "fan2d_70", "knife_rot90_2d", "knife_rot90_3d", "mirror_swap", "mirror_swap_one_rotated",
         "shear_aniso", "trimmed", "far_origin")


def _tile(data, spacing, origin):
    from multiview_stitcher_amd import spatial_image_utils as si

    sd = SDIMS[-data.ndim:]
    sim = si.get_sim_from_array(data, dims=sd, scale=dict(zip(sd, (float(v) for v in spacing))),
                                translation=dict(zip(sd, (float(v) for v in origin))))
    return squeeze_field(sim)


def _about(lin, centre, shift=0.0):
    """The world map x -> lin (x - centre) + centre + shift as a homogeneous matrix."""
    lin, centre = np.asarray(lin, np.float64), np.asarray(centre, np.float64)
    n = len(centre)
    p = np.eye(n + 1)
    p[:n, :n] = lin
    p[:n, n] = centre - lin @ centre + shift
    return p


def rot_yx(ndim, angle):
    """Rotation in the yx plane, its entries straight from np.cos / np.sin (np.pi / 2 leaves cos = 6.1e-17)."""
    r = np.eye(ndim)
    c, s = np.cos(angle), np.sin(angle)
    r[-2:, -2:] = [[c, -s], [s, c]]
    return r


def _centre(shape, spacing, origin):
    return np.asarray(origin, np.float64) + (np.asarray(shape) - 1) / 2.0 * np.asarray(spacing, np.float64)


def _union(sims, params, spacing):
    _, bbs = zip(*[sim_to_view(s) for s in sims])
    return union_bb(bbs, params, np.asarray(spacing, np.float64))


def _fan(shape, n, dtype, seed, shift):
    ndim = len(shape)
    rng, geo = np.random.default_rng(seed), np.random.default_rng(seed + 100)      # (the shifts do not depend on the dtype)
    c = _centre(shape, np.ones(ndim), np.zeros(ndim))
    sims = [_tile(white_noise(rng, shape, dtype), np.ones(ndim), np.zeros(ndim)) for _ in range(n)]
    params = [_about(rot_yx(ndim, 2 * np.pi * i / n), c, geo.uniform(-shift, shift, ndim) if shift else 0.0) for i in range(n)]
    return sims, params, _union(sims, params, np.ones(ndim)), {}


def _positive(rng, shape, dtype):
    """White noise without a zero: the fused value of a voxel is 0 exactly where no view is in bounds."""
    a = white_noise(rng, shape, dtype)
    return (a * 0.9 + 0.1).astype(np.float32) if np.dtype(dtype).kind == "f" else np.maximum(a, 1)


def _knife_rot90(ndim, dtype):
    """Identity, a turn by exactly np.pi / 2 (np.cos leaves 6.1e-17 in the matrix) and one by np.pi, about the tile centre, moved by
    whole input voxels.  The pixel matrices go through the reference's rounding to 10 decimals (transformation.py:72-83), which takes
    the 6.1e-17 away -- with equal spacings these views would have exact permutation matrices (that is ``mirror_swap``).  Here the
    input spacing is 1.5 and the output spacing 0.5 in y and x: the matrix entry 1 / 3 is rounded to 0.3333333333, every view border
    lies on an output voxel 3 k, and the coordinate there is an integer -+ k * 1e-10: below 0 or above n - 1 for one sign, inside
    for the other.  The sum's order and the absence of an fma decide the last bit of such a coordinate."""
    rng = np.random.default_rng(21 + ndim)
    n = 26 if ndim == 2 else 22
    shape = (n, n) if ndim == 2 else (6, n, n)
    spacing = np.array([1.0, 1.5, 1.5][-ndim:])
    c = _centre(shape, spacing, np.zeros(ndim))
    sims = [_tile(_positive(rng, shape, dtype), spacing, np.zeros(ndim)) for _ in range(3)]
    shifts = [np.zeros(3), np.array([1.0, 3.0, -1.5]), np.array([-1.0, -1.5, 3.0])]
    params = [_about(rot_yx(ndim, a), c, s[-ndim:]) for a, s in zip((0.0, np.pi / 2, np.pi), shifts)]
    out_spacing = np.array([1.0, 0.5, 0.5][-ndim:])
    if ndim == 2:
        out_bb = fo.bb([-6.0, -6.0], out_spacing, (90, 90))
    else:
        out_bb = fo.bb([-2.0, -4.5, -4.5], out_spacing, (10, 78, 78))
    return sims, params, out_bb, {}


MIRROR_SHAPE = (8, 30, 44)


def _mirror_swap(dtype, one_rotated=False):
    rng = np.random.default_rng(31)
    shape = MIRROR_SHAPE
    tiles = []
    for _ in range(4):
        a = white_noise(rng, shape, dtype)
        if np.dtype(dtype).kind == "f":
            a[tuple(rng.integers(0, n, 60) for n in shape)] = np.nan
            for axis, n in enumerate(shape):          # the mirrored second tap of the last voxel, along every axis
                idx = [rng.integers(0, m) for m in shape]
                idx[axis] = n - 2
                a[tuple(idx)] = np.nan
            a[tuple(n - 2 for n in shape)] = np.nan
        tiles.append(a)
    sims = [_tile(a, np.ones(3), np.zeros(3)) for a in tiles]
    swap = np.array([[1.0, 0, 0], [0, 0, 1], [0, 1, 0]])
    lins = [np.eye(3), swap, np.diag([1.0, 1.0, -1.0]), -np.eye(3)]
    offs = [np.zeros(3), np.array([1.0, 5.0, -7.0]), np.array([0.0, 12.0, 63.0]), np.array([9.0, 23.0, 52.0])]
    if one_rotated:
        offs = [np.zeros(3), np.array([1.0, 5.0, 14.0]), np.array([0.0, 12.0, 20.0]), np.array([2.0, -6.0, 9.0])]
        c = _centre(shape, np.ones(3), np.zeros(3))
        params = [_about(np.eye(3), c, o) for o in offs[:3]] + [_about(rot_yx(3, np.deg2rad(30.0)), c, offs[3])]
    else:
        params = []
        for lin, o in zip(lins, offs):
            p = np.eye(4)
            p[:3, :3], p[:3, 3] = lin, o
            params.append(p)
    return sims, params, _union(sims, params, np.ones(3)), {}


SHEAR_IN_SPACING = np.array([2.0, 0.8, 1.3])
SHEAR_OUT_SPACING = np.array([1.0, 0.75, 1.25])
SHEAR_CORNER_VIEW = 2
# where the third view sits: its nearest corner reaches two voxels into the far (y, x) corner of the chunk
SHEAR_CORNER_SHIFT = np.array([0.5, 46.0, 62.0])


def _shear_aniso(dtype, trim=0):
    rng = np.random.default_rng(41)
    shape = (6, 48, 40)
    sims = [_tile(white_noise(rng, shape, dtype), SHEAR_IN_SPACING, o) for o in ([0.0, 0.0, 0.0], [1.0, 6.4, 13.0], [0.0, 0.0, 0.0])]
    c = _centre(shape, SHEAR_IN_SPACING, np.zeros(3))
    lin0 = np.array([[1.0, 0.02, 0.0], [0.03, 1.05, 0.08], [0.0, -0.06, 0.95]])
    lin1 = np.array([[1.0, 0.0, -0.02], [0.0, 0.92, -0.07], [0.04, 0.05, 1.1]]) @ np.diag([1.0, 1.0, -1.0])      # determinant < 0
    lin2 = rot_yx(3, np.deg2rad(25.0)) @ np.diag([1.0, 1.08, 0.93])
    params = [_about(lin0, c, [0.3, 1.7, -2.2]), _about(lin1, c + [1.0, 6.4, 13.0], [-0.4, -3.1, 4.6]),
              _about(lin2, c, SHEAR_CORNER_SHIFT)]
    out_bb = fo.bb([-1.5, -3.0, -4.0], SHEAR_OUT_SPACING, (12, 72, 63))
    return sims, params, out_bb, ({"trim_overlap_in_pixels": trim} if trim else {})


def _far_origin(dtype):
    rng = np.random.default_rng(51)
    shape = (6, 36, 48)
    origins = [np.array([100000.0, 99990.5, 100020.25]), np.array([100001.0, 100002.75, 100031.5])]
    sims = [_tile(white_noise(rng, shape, dtype), np.ones(3), o) for o in origins]
    params = [_about(rot_yx(3, np.deg2rad(a)), _centre(shape, np.ones(3), o), s)
              for a, o, s in zip((17.0, -33.0), origins, ([0.3, -1.2, 0.7], [-0.6, 0.4, -1.9]))]
    return sims, params, _union(sims, params, np.ones(3)), {}


@functools.lru_cache(maxsize=None)
def _build(name, dtype):
    if name == "fan3d_12":
        return _fan((9, 30, 70), 12, dtype, 11, 2.0)
    if name == "fan2d_12":
        return _fan((40, 70), 12, dtype, 12, 2.0)
    if name == "fan2d_70":
        return _fan((24, 40), 70, dtype, 13, 0.0)
    if name == "knife_rot90_2d":
        return _knife_rot90(2, dtype)
    if name == "knife_rot90_3d":
        return _knife_rot90(3, dtype)
    if name == "mirror_swap":
        return _mirror_swap(dtype)
    if name == "mirror_swap_one_rotated":
        return _mirror_swap(dtype, one_rotated=True)
    if name == "shear_aniso":
        return _shear_aniso(dtype)
    if name == "trimmed":
        return _shear_aniso(dtype, trim=3)
    if name == "far_origin":
        return _far_origin(dtype)
    raise KeyError(name)


def build(name, dtype=np.uint16):
    """The case ``name`` with tiles of ``dtype``: (sims, params, out_bb, kwargs).  Built once per (name, dtype); leave it unchanged."""
    return _build(name, np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _oracle(name, dtype, fusion, order):
    sims, params, out_bb, kw = _build(name, dtype)
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    return fo.fuse_np(list(views), list(params), out_bb, fusion=fusion, full_view_bbs=list(bbs), interpolation_order=order,
                      return_debug=True, **kw)


def oracle(name, dtype=np.uint16, fusion="weighted_average", order=1):
    """``fo.fuse_np(..., return_debug=True)`` of a case: (fused, fused float32, debug).  Computed once; leave it unchanged."""
    return _oracle(name, np.dtype(dtype), fusion, order)
