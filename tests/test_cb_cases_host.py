"""The preconditions of the content-based cases (tests/cb_cases.py), checked with the oracle alone: every case takes the route it is
listed for, and the oracle and the device classify every voxel of it alike.  A case that fails here gets another seed, shift or
shape; it is never skipped or dropped."""
import numpy as np
import pytest

from oracle import fuse_oracle as fo
from tests import cb_cases as cc
from tests.helpers import sim_to_view

CELLS = cc.cells()
# every check of the default path that declines the chunk, in the order csrc/mvs_cb_plan.h makes them (the first one is the one that
# fires); cases not listed here are declined by the one check they are in the table for
ALSO = {"fan2d_12": ["kCbViewCount", "kCbMatrix"], "fan3d_12": ["kCbViewCount", "kCbMatrix"], "far_origin": ["kCbShortAxis", "kCbMatrix"]}


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_is_declined_for_the_reason_it_names(name):
    plan = cc.plan(name)
    assert cc.REASON[name] in plan["reasons"]
    assert plan["reasons"] == ALSO.get(name, [cc.REASON[name]]), plan


def test_routes_of_the_bit_faithful_passes():
    """Which kernels the plan sends each case to (the GPU test reads the same numbers back from the library's counters)."""
    for name in cc.NAMES:
        plan, nv = cc.plan(name), len(cc.build(name)[0])
        ndim, live = len(cc.build(name)[2]["shape"]), nv - len(cc.ABSENT.get(name, ()))
        c = plan["counters"]
        assert c["cb_exact_large_chunks"] == int(name in ("fan2d_12", "fan3d_12", "nine_views_3d")), name
        if name in ("long_y", "mid_y"):
            assert c["cb_exact_paired_launches"] == 0 and c["cb_exact_lds_launches"] + c["cb_exact_tap_launches"] == 4 * ndim * live
        else:
            assert c == dict(c, cb_exact_paired_launches=2 * ndim * live, cb_exact_lds_launches=0, cb_exact_tap_launches=0), (name, c)
    # long_y: no tile of either kind holds a y line (tap by tap along y, LDS-staged along x); mid_y: a single tile does, a paired one not
    assert cc.plan("long_y")["counters"]["cb_exact_tap_launches"] == cc.plan("long_y")["counters"]["cb_exact_lds_launches"] == 8
    assert cc.plan("mid_y")["counters"]["cb_exact_tap_launches"] == 0 and cc.plan("mid_y")["counters"]["cb_exact_lds_launches"] == 16
    for name, lo, hi in (("long_y", 1706, 10 ** 9), ("mid_y", 1536, 1706)):
        plan = cc.plan(name)
        for box in plan["boxes"]:
            for r in plan["radii"]:
                assert lo < box[1] + 2 * r <= hi, (name, box, r)
                assert cc.pair_T(box[1], r, 1) == 0 and bool(cc.single_T(box[1], r, 1)) == (name == "mid_y")
                assert cc.pair_T(box[2], r, 2) > 0 and cc.single_T(box[2], r, 2) > 0


def test_short_axes_are_as_short_as_they_say():
    r1, r2 = cc.radius(1.5), cc.radius(3.0)
    assert (r1, r2) == (6, 12) and (cc.radius(1.0), cc.radius(2.0), cc.radius(5.0), cc.radius(11.0), cc.radius(32.0)) == (4, 8, 20, 44, 128)
    assert cc.plan("short_z3")["chunk"][0] < r1                      # both filters bounce several times
    assert r1 <= cc.plan("short_z7")["chunk"][0] < r2
    assert cc.plan("one_plane")["chunk"][0] == 1 and len(cc.build("one_plane")[2]["shape"]) == 3      # box_reflect's full == 1 branch
    assert 20 <= cc.plan("short_z_default")["chunk"][0] < 44 and cc.build("short_z_default")[3] == (5.0, 11.0)
    assert r1 <= cc.plan("short_y_2d")["chunk"][1] < r2 and len(cc.build("short_y_2d")[2]["shape"]) == 2
    stray = cc.plan("stray_views")
    assert 4 <= stray["chunk"][0] < 8 and stray["radii"] == (4, 8)
    assert stray["boxes"][cc.STRAY_OUTSIDE] == (0, 0, 0) and stray["boxes"][cc.STRAY_ROW][1] == 1 and stray["boxes"][cc.STRAY_ROW][2] > 1
    assert cc.ABSENT["stray_views"] == (cc.STRAY_OUTSIDE,)
    big = cc.plan("radius_128")
    assert max(big["radii"]) == 128 and min(big["chunk"][1:]) >= 128 and cc.build("radius_128")[4] == {"trim_overlap_in_pixels": 64}


def test_chunks_stay_small():
    for name in cc.NAMES:
        assert int(np.prod(cc.plan(name)["chunk"])) <= 200000, name


def test_rotated_cases_have_boxes_that_start_inside_the_chunk_and_masks_that_are_no_boxes():
    for name in ("shear_aniso", "lightsheet_pair", "fan3d_12"):
        views = cc.oracle(name, cc.U16)[2]["views"]
        inside = not_box = 0
        for v in views:
            inb = ~np.isnan(v)
            idx = np.argwhere(inb)
            inside += int((idx.min(0) > 0).any())
            not_box += int(inb.sum() != np.prod(idx.max(0) - idx.min(0) + 1))
        assert inside >= 1 and not_box >= 1, (name, inside, not_box)
    # the corner view of shear_aniso: lines of one or two samples
    corner = ~np.isnan(cc.oracle("shear_aniso", cc.U16)[2]["views"][2])
    per_line = corner.sum(-1)
    assert 1 <= per_line[per_line > 0].min() <= 2


@pytest.mark.parametrize("cell", CELLS, ids=cc.cell_id)
def test_weights_keep_a_margin_from_the_threshold(cell):
    """Every raw blending weight of the oracle is exactly 0 or at least 1e-5: the oracle's cosine ramp carries about 6e-8 of absolute
    float32 noise (helpers.reference_noise_floor), the device's sin^2 ramp does not, and content_based sets a view to NaN where its
    normalised weight is below 1e-7 -- with the margin both sides take every voxel of every view for the same side of that."""
    name, dtype, order = cell
    w = cc.oracle(name, dtype, order)[2]["raw_weights"]
    pos = w[w > 0]
    assert np.all(w >= 0) and pos.size and pos.min() >= 1e-5, (float(pos.min()), int((pos < 1e-5).sum()))


def _coordinates(name, iv):
    """Sampling coordinates of view ``iv`` over the chunk (float64), the view's shape, and per view axis whether its matrix row and
    offset are multiples of 1 / 1024: the coordinates along such an axis are exact however they are summed."""
    sims, params, out_bb, _, _ = cc.build(name, cc.U16)
    view, bb = sim_to_view(sims[iv])
    m, o = fo.transform_params(np.linalg.inv(params[iv]), view["origin"], bb["spacing"], out_bb)
    grid = np.stack(np.meshgrid(*[np.arange(int(n), dtype=np.float64) for n in out_bb["shape"]], indexing="ij"))
    coords = np.tensordot(m, grid, axes=1) + o.reshape((-1,) + (1,) * len(o))
    exact = np.all(m * 1024 == np.round(m * 1024), axis=1) & (o * 1024 == np.round(o * 1024))
    return coords, view["data"].shape, exact


@pytest.mark.parametrize("name", cc.NAMES)
def test_coordinates_keep_a_margin_from_borders_and_half_integers(name):
    """No sampling coordinate within 1e-6 of a view border (where in-bounds changes) and, for the cases that run at order 0, of a
    half-integer (where the nearest voxel changes; looked for where the view is sampled: inside it and one voxel around) -- the
    condition of tests/test_masks_gpu.py::check_fuse.  Exempt is a view axis whose matrix row and offset are multiples of 1 / 1024:
    its coordinates are exact on either side, equal to the borders where they meet them, and ties go one way (mirror_swap; the z axis
    of shear_aniso's corner view, z / 2 - 1; the view whose corner is the origin of a union box, after the reference's snap of
    offsets within 1e-6 of an integer)."""
    orders = {o for n, _, o in CELLS if n == name}
    n_exact = 0
    for iv in range(len(cc.build(name)[0])):
        c, shape, exact = _coordinates(name, iv)
        near = np.all([(c[k] > -1.0) & (c[k] < n) for k, n in enumerate(shape)], axis=0)
        for k, n in enumerate(shape):
            if exact[k]:
                n_exact += 1
                assert np.array_equal(c[k] * 1024, np.round(c[k] * 1024))
                continue
            assert min(np.abs(c[k]).min(), np.abs(c[k] - (n - 1)).min()) > 1e-6, (iv, k)
            if 0 in orders and near.any():
                assert np.abs(c[k][near] - np.floor(c[k][near]) - 0.5).min() > 1e-6, (iv, k)
    assert n_exact <= len(shape) or name.startswith("mirror_swap"), n_exact


@pytest.mark.parametrize("cell", CELLS, ids=cc.cell_id)
def test_case_is_live_and_the_noise_floor_is_rarely_needed(cell):
    name, dtype, order = cell
    fused, fused_f, dbg, floor = cc.oracle(name, dtype, order)
    assert float((fused != 0).mean()) >= 0.30
    for iv, v in enumerate(dbg["views"]):
        assert bool(np.isfinite(v).any()) == (iv not in cc.ABSENT.get(name, ())), iv
    if np.dtype(dtype).kind == "f":
        bar = 1e-4 * np.maximum(np.abs(fused_f), 1e-3 * float(np.abs(fused_f).max()))
    else:
        bar = 1e-4 * np.maximum(np.abs(fused_f), 1.0)
    frac = float((floor > bar).mean())
    assert frac <= 0.01, frac
