"""The preconditions of the affine cases (tests/affine_cases.py), checked with the oracle alone: every case reaches the branch of the
generic fuse kernel it is built for.  A case that fails here gets another seed, shift or shape; it is never skipped or dropped."""
import numpy as np
import pytest

from tests import affine_cases as ac
from tests.helpers import sim_to_view


def _in_bounds(name):
    """(views, trimmed chunk) booleans: the oracle's in-bounds classification (uint16 tiles: no NaN but cval)."""
    _, _, dbg = ac.oracle(name, np.uint16)
    inb = ~np.isnan(dbg["views"])
    sl = (slice(None),) + tuple(slice(t, -t) if t > 0 else slice(None) for t in dbg["trim"])
    return inb[sl]


def _views_per_brick(name):
    """Per brick of the generic kernel the number of views with an in-bounds voxel.  The brick is the one of csrc/mvs_fuse_chunk_plan.h
    (kBrickX = 64 voxels along x; brick_grid(kGenericBricks): 4 x 4 in z, y for a 3D result, 1 x 16 for a 2D one), counted in the index of
    the trimmed result.  The kernel's cull (brick_hits_view) is conservative, so it lists at least these views."""
    inb = _in_bounds(name)
    if inb.ndim == 3:
        inb = inb[:, None]
    brick = (4, 4, 64) if inb.shape[1] > 1 else (1, 16, 64)
    pad = [(0, 0)] + [(0, -n % b) for n, b in zip(inb.shape[1:], brick)]
    inb = np.pad(inb, pad)
    v, z, y, x = inb.shape
    hit = inb.reshape(v, z // brick[0], brick[0], y // brick[1], brick[1], x // brick[2], brick[2]).any(axis=(2, 4, 6))
    return hit.sum(0)


@pytest.mark.parametrize("name,more_than", [("fan3d_12", 8), ("fan2d_12", 8), ("fan2d_70", 64)])
def test_fan_has_a_brick_with_more_views_than_a_pass_holds(name, more_than):
    """More than 8: the 9th active view of a brick reads its 5^n table from global memory (kLdsTables = 8); more than 64: the brick
    has active views in the second cull batch."""
    per_brick = _views_per_brick(name)
    assert per_brick.max() > more_than, per_brick.max()
    per_voxel = _in_bounds(name).sum(0)
    assert per_voxel.max() > more_than          # ... and they meet at a voxel, so the late views carry weight there
    if name == "fan2d_70":
        assert per_voxel.max() == 70


def test_cases_have_the_layouts_they_name():
    assert len(ac.build("fan3d_12")[0]) == len(ac.build("fan2d_12")[0]) == 12 and len(ac.build("fan2d_70")[0]) == 70
    assert [int(v) for v in ac.build("fan2d_12")[2]["shape"]][0] > 16        # more than one 2D brick along y
    for name in ac.NAMES:
        shape = [int(v) for v in ac.build(name)[2]["shape"]]
        assert (len(shape) == 2 and max(shape) <= 90) or (shape[0] <= 13 and max(shape[1:]) <= 80), (name, shape)


def _coordinates(name, iv):
    """Input coordinates of view ``iv`` at every voxel of the chunk: float64, in the order the kernel states and scipy uses,
    ((z * m0 + y * m1) + x * m2) + offset, no fused multiply-add.  Returns (coords (ndim, *chunk), view shape)."""
    from multiview_stitcher_amd import transformation

    sims, params, out_bb, _ = ac.build(name, np.uint16)
    view, bb = sim_to_view(sims[iv])
    m, o = transformation.get_pixel_affine(np.linalg.inv(params[iv]), view["origin"], bb["spacing"], out_bb["origin"], out_bb["spacing"])
    grid = np.meshgrid(*[np.arange(int(n), dtype=np.float64) for n in out_bb["shape"]], indexing="ij")
    coords = []
    for d in range(len(grid)):
        acc = grid[0] * m[d, 0]
        for k in range(1, len(grid)):
            acc = acc + grid[k] * m[d, k]
        coords.append(acc + o[d])
    return np.stack(coords), np.asarray(view["data"].shape)


def _classified(coords, shape):
    hi = (shape - 1).reshape((-1,) + (1,) * (coords.ndim - 1))
    return np.all((coords >= 0) & (coords <= hi), axis=0)


@pytest.mark.parametrize("name", ["knife_rot90_2d", "knife_rot90_3d"])
def test_knife_case_has_coordinates_an_ulp_from_the_border(name):
    """Output voxels whose coordinate lies within 1e-9 of 0 or n - 1 without being equal to it, some of which the oracle puts out of
    bounds: the residue decides.  Others lie as close on the inner side (k * 1e-10 with k up to 29: counted within 1e-8) and stay in
    bounds.  The stated operation order reproduces the oracle's mask voxel for voxel."""
    _, _, dbg = ac.oracle(name, np.uint16)
    knife_out = knife_in = 0
    for iv in range(3):
        coords, shape = _coordinates(name, iv)
        oracle_in = ~np.isnan(dbg["views"][iv])
        np.testing.assert_array_equal(_classified(coords, shape), oracle_in)
        for d in range(coords.shape[0]):
            others = _classified(np.delete(coords, d, axis=0), np.delete(shape, d))
            for bound in (0.0, float(shape[d] - 1)):
                near = (np.abs(coords[d] - bound) < 1e-9) & (coords[d] != bound) & others
                knife_out += int((near & ~oracle_in).sum())
                near_in = (np.abs(coords[d] - bound) < 1e-8) & (coords[d] != bound) & others
                knife_in += int((near_in & oracle_in).sum())
    assert knife_out >= 1 and knife_in >= 1, (knife_out, knife_in)


def test_knife_case_holds_the_turn_by_half_pi_with_its_residue():
    for name in ("knife_rot90_2d", "knife_rot90_3d"):
        p = ac.build(name)[1][1]
        assert abs(p[-3, -3]) == np.cos(np.pi / 2) > 0 and p[-2, -3] == 1.0


def test_mirror_swap_has_coordinates_equal_to_the_bounds():
    from multiview_stitcher_amd import transformation

    sims, params, out_bb, _ = ac.build("mirror_swap", np.uint16)
    _, _, dbg = ac.oracle("mirror_swap", np.uint16)
    for iv in range(4):
        view, bb = sim_to_view(sims[iv])
        m, _ = transformation.get_pixel_affine(np.linalg.inv(params[iv]), view["origin"], bb["spacing"], out_bb["origin"], out_bb["spacing"])
        assert np.all(np.isin(m, (-1.0, 0.0, 1.0))) and np.all(np.abs(m).sum(0) == 1) and np.all(np.abs(m).sum(1) == 1)
        coords, shape = _coordinates("mirror_swap", iv)
        inb = _classified(coords, shape)
        np.testing.assert_array_equal(inb, ~np.isnan(dbg["views"][iv]))
        for d in range(3):
            assert (inb & (coords[d] == 0.0)).any() and (inb & (coords[d] == shape[d] - 1)).any(), (iv, d)
    assert not np.array_equal(params[1][:3, :3], np.eye(3)) and np.linalg.det(params[2][:3, :3]) == -1


def test_mirror_swap_float_tiles_hold_nan_at_the_mirrored_tap():
    sims = ac.build("mirror_swap", np.float32)[0]
    for s in sims:
        d = np.asarray(s.data)
        assert np.isnan(d[tuple(n - 2 for n in d.shape)]) and 50 < np.isnan(d).sum() < 80
        for axis, n in enumerate(d.shape):
            assert np.isnan(np.take(d, n - 2, axis=axis)).sum() >= 2


def test_one_rotated_case_has_three_identity_pixel_matrices():
    from multiview_stitcher_amd import transformation

    sims, params, out_bb, _ = ac.build("mirror_swap_one_rotated", np.uint16)
    ident = []
    for s, p in zip(sims, params):
        view, bb = sim_to_view(s)
        m, o = transformation.get_pixel_affine(np.linalg.inv(p), view["origin"], bb["spacing"], out_bb["origin"], out_bb["spacing"])
        ident.append(bool(np.array_equal(m, np.eye(3))))
    assert ident == [True, True, True, False]


def test_shear_aniso_is_sheared_and_its_third_view_touches_with_a_corner():
    sims, params, out_bb, _ = ac.build("shear_aniso", np.uint16)
    dets = [np.linalg.det(p[:3, :3]) for p in params]
    assert dets[1] < 0 < dets[0] and all(0.8 < abs(d) < 1.25 for d in dets)
    assert all(np.count_nonzero(p[:3, :3]) >= 5 for p in params)
    np.testing.assert_array_equal(sim_to_view(sims[0])[0]["spacing"], ac.SHEAR_IN_SPACING)
    np.testing.assert_array_equal(out_bb["spacing"], ac.SHEAR_OUT_SPACING)
    per_view = _in_bounds("shear_aniso").reshape(3, -1).sum(1)
    assert 1 <= per_view[ac.SHEAR_CORNER_VIEW] <= 64, per_view
    assert per_view[:2].min() > 10000
    where = np.argwhere(_in_bounds("shear_aniso")[ac.SHEAR_CORNER_VIEW])
    assert np.all(where[:, 1:].min(0) >= np.asarray(out_bb["shape"])[1:] - 4)      # the far (y, x) corner of the chunk


def test_trimmed_width_is_no_multiple_of_four():
    sims, params, out_bb, kw = ac.build("trimmed", np.uint16)
    fused = ac.oracle("trimmed", np.uint16)[0]
    assert kw == {"trim_overlap_in_pixels": 3}
    assert fused.shape == tuple(int(n) - 6 for n in out_bb["shape"]) and fused.shape[-1] % 4 != 0
    for a, b in zip(ac.build("shear_aniso")[1], params):
        np.testing.assert_array_equal(a, b)


def test_far_origin_views_lie_near_1e5_and_are_turned():
    sims, params, out_bb, _ = ac.build("far_origin", np.uint16)
    for s, p in zip(sims, params):
        assert np.all(np.abs(sim_to_view(s)[0]["origin"]) > 9e4) and abs(p[1, 2]) > 0.2
    assert np.all(np.abs(out_bb["origin"]) > 9e4)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("name", ac.NAMES)
def test_case_is_neither_empty_nor_full(name, dtype):
    fused = ac.oracle(name, dtype)[0]
    frac = float((fused != 0).mean())
    assert 0.30 <= frac <= 0.95, frac
