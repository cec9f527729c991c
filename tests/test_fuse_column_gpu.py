"""GPU parity of the COLUMN kernel of mvs_fuse_chunk (fuse_tr_kernel / xweight_table_kernel in csrc/mvs_fuse.hip) against the
oracle's fuse_np, on the paths only it takes.

The column kernel fuses translated tiles when the region planner declines a weighted-average chunk (more than 8 views on a cell,
too many cells or regions, option "no_regions") and it fuses every ``max`` / ``simple_average`` chunk of translated tiles.  The
cases run with DEFAULT options unless they say otherwise: dense mosaics reach the kernel the way production does.  Every case
resets the counters "fuse_*_chunks", and asserts afterwards that the column kernel fused the chunk and no other family ran.

Shapes: the smallest that reach each edge -- an output row longer than one 256-voxel segment with a ragged last segment, more
rows than the 128 one 2-D workgroup owns, a z extent that is no multiple of the 4 planes of a 3-D workgroup, more than 16 views
on one column (a second round of candidates), windows that straddle the first / last byte of a slab.  Bars: the defaults of
``assert_fused_close``; ``assert_array_equal`` where one view decides a voxel."""
import numpy as np
import pytest

from oracle import fuse_oracle as fo
from tests.helpers import assert_fused_close, bb_to_dicts, grid_case, reference_noise_floor, run_both, sim_to_view, union_bb

pytestmark = pytest.mark.gpu

FAMILIES = ("fuse_rows_chunks", "fuse_region_chunks", "fuse_column_chunks", "fuse_generic_chunks")

# the dense mosaics: tiles, tile shape, overlap.  Steps of (12, 34), (20, 46) and (4, 8, 13) voxels: up to 4 x 4 = 16, 5 x 3 = 15
# and 3 x 3 x 3 = 27 views on one voxel
GRID_2D = ((4, 5), (48, 136), (36, 102))
GRID_2D_TALL = ((6, 3), (100, 136), (80, 90))
GRID_3D = ((3, 3, 3), (12, 24, 40), (8, 16, 27))


def _reset_counters():
    from multiview_stitcher_amd import _lib

    for key in FAMILIES:
        _lib.get_counter(key, reset=True)


def _assert_only(family):
    """The chunk(s) since the last reset were fused by ``family`` and by nothing else."""
    from multiview_stitcher_amd import _lib

    counts = {key: _lib.get_counter(key, reset=True) for key in FAMILIES}
    assert counts[family] >= 1 and all(v == 0 for k, v in counts.items() if k != family), counts


def _dense_case(ndim, dtype, frac_shift, grid=None, seed=0):
    tiles, shape, overlap = grid or (GRID_2D if ndim == 2 else GRID_3D)
    sims, params = grid_case(ndim, dtype, tiles, shape, overlap, frac_shift, seed=seed)
    if dtype == np.uint8:
        sims = [s.copy(data=(np.asarray(s.data) >> 4).astype(np.uint8)) for s in sims]
    _, bbs = zip(*[sim_to_view(s) for s in sims])
    return sims, params, union_bb(bbs, params, np.ones(ndim))


def _max_views_on_a_voxel(sims, params, out_bb):
    """Largest number of views whose (translated) box covers one output voxel."""
    count = np.zeros(tuple(int(n) for n in out_bb["shape"]), np.int32)
    for s, p in zip(sims, params):
        _, vbb = sim_to_view(s)
        nd = len(vbb["shape"])
        lo = (vbb["origin"] + p[:nd, nd] - out_bb["origin"]) / out_bb["spacing"]
        hi = lo + (vbb["shape"] - 1) * vbb["spacing"] / out_bb["spacing"]
        count[tuple(slice(int(np.ceil(a)), int(np.floor(b)) + 1) for a, b in zip(lo, hi))] += 1
    return int(count.max())


def _fuse_on_column(sims, params, out_bb, **kw):
    """run_both with the counters around it: the column kernel fused the chunk, no other family ran."""
    _reset_counters()
    got, want, (want_f, floor) = run_both(sims, params, out_bb, **kw)
    _assert_only("fuse_column_chunks")
    return got, want, want_f, floor


@pytest.mark.parametrize("switch,family", [(None, "fuse_region_chunks"), ("rows_v1", "fuse_rows_chunks"),
                                           ("force_generic", "fuse_generic_chunks"), ("no_regions", "fuse_column_chunks")])
def test_counters_name_the_family_that_fused(hip_device, switch, family):
    """The counters themselves: a sparse 2 x 3 mosaic goes to the region kernels by default and to the family a switch names."""
    from multiview_stitcher_amd import _lib

    sims, params = grid_case(2, np.uint16, (2, 3), (40, 72), 9, True)
    _, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = union_bb(bbs, params, np.ones(2))
    if switch:
        _lib.set_option(switch, 1)
    try:
        _reset_counters()
        got, want, (want_f, floor) = run_both(sims, params, out_bb)
        _assert_only(family)
    finally:
        if switch:
            _lib.set_option(switch, 0)
    assert_fused_close(got, want, want_f, noise_floor=floor)


# ---- a. weighted average, more than 8 views on a cell: the region planner declines, the column kernel fuses ----

@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("frac_shift", [False, True])
def test_weighted_average_2d_20_views(hip_device, dtype, frac_shift):
    """Rows of 272 (275) voxels: a whole 256-voxel segment and a ragged one; 16 views on a voxel: one full round of candidates."""
    sims, params, out_bb = _dense_case(2, dtype, frac_shift)
    assert len(sims) == 20 and _max_views_on_a_voxel(sims, params, out_bb) > 8
    got, want, want_f, floor = _fuse_on_column(sims, params, out_bb)
    assert got.shape[1] > 256 and got.shape[1] % 256 and (frac_shift or got.shape == (84, 272))
    assert_fused_close(got, want, want_f, noise_floor=floor)


@pytest.mark.parametrize("frac_shift", [False, True])
def test_weighted_average_2d_20_views_float32_order0(hip_device, frac_shift):
    """float32 tiles reach the column kernel at order 0 only (at order 1 the row kernels take them)."""
    sims, params, out_bb = _dense_case(2, np.float32, frac_shift)
    got, want, want_f, floor = _fuse_on_column(sims, params, out_bb, interpolation_order=0)
    assert_fused_close(got, want, want_f, noise_floor=floor)


def test_weighted_average_2d_18_views_tall(hip_device):
    """201 rows: more than the 128 rows of one 2-D workgroup (4 wavefronts x 32 rows), the last row group ragged."""
    sims, params, out_bb = _dense_case(2, np.uint16, True, grid=GRID_2D_TALL)
    assert len(sims) == 18 and _max_views_on_a_voxel(sims, params, out_bb) > 8
    got, want, want_f, floor = _fuse_on_column(sims, params, out_bb)
    assert got.shape[0] > 128 and got.shape[0] % 32
    assert_fused_close(got, want, want_f, noise_floor=floor)


@pytest.mark.parametrize("dtype,frac_shift", [(np.uint16, True), (np.uint8, False)])
def test_weighted_average_3d_27_views(hip_device, dtype, frac_shift):
    """More than 16 views on one column: the candidate loop takes a second round.  Fractional offsets: 23 planes, no multiple of the
    4 planes of a workgroup (integer offsets: 20)."""
    sims, params, out_bb = _dense_case(3, dtype, frac_shift)
    assert len(sims) == 27 and _max_views_on_a_voxel(sims, params, out_bb) > 16
    got, want, want_f, floor = _fuse_on_column(sims, params, out_bb)
    assert got.shape[0] % 4 if frac_shift else got.shape == (20, 40, 66)
    assert_fused_close(got, want, want_f, noise_floor=floor)


def test_weighted_average_2d_20_views_trimmed(hip_device):
    sims, params, out_bb = _dense_case(2, np.uint16, True)
    got, want, want_f, floor = _fuse_on_column(sims, params, out_bb, trim_overlap_in_pixels=3)
    assert got.shape == tuple(out_bb["shape"] - 6)
    assert_fused_close(got, want, want_f, noise_floor=floor)


# ---- b. max / simple_average: always the column kernel ----

@pytest.mark.parametrize("fusion_name", ["max", "simple_average"])
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("frac_shift", [False, True])
def test_max_and_simple_average_dense(hip_device, fusion_name, ndim, dtype, frac_shift):
    """Integer offsets: the single-tap branch (4-element windows); fractional: 5-element windows (5 bytes for uint8)."""
    sims, params, out_bb = _dense_case(ndim, dtype, frac_shift)
    got, want, want_f, floor = _fuse_on_column(sims, params, out_bb, fusion=fusion_name)
    assert_fused_close(got, want, want_f, noise_floor=floor)


@pytest.mark.parametrize("fusion_name", ["max", "simple_average"])
@pytest.mark.parametrize("frac_shift", [False, True])
def test_max_and_simple_average_float32_order0_drop_nan(hip_device, fusion_name, frac_shift):
    """float32 tiles at order 0, two of them with a handful of NaN voxels: a NaN drops the view from that voxel (nanmax / nansum over
    the views that are left) and never reaches the output."""
    sims, params, out_bb = _dense_case(2, np.float32, frac_shift)
    rng = np.random.default_rng(11)
    for i in (6, 13):
        d = np.array(sims[i].data, dtype=np.float32, copy=True)
        d[tuple(rng.integers(0, n, 12) for n in d.shape)] = np.nan
        d[0, 0] = d[-1, -1] = np.nan
        sims[i] = sims[i].copy(data=d)
    got, want, want_f, floor = _fuse_on_column(sims, params, out_bb, fusion=fusion_name, interpolation_order=0)
    assert np.isfinite(got).all()
    assert_fused_close(got, want, want_f, noise_floor=floor)


# ---- c. slab ends, exact ----

@pytest.mark.parametrize("shape", [(3, 37, 261), (37, 261)])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("shifted", [False, True])
def test_single_view_slab_ends_are_exact(hip_device, shape, dtype, shifted):
    """One view on its own grid through the column kernel ("no_regions").  Rows of 261 voxels: the window of the last lane of
    every row's second segment runs past the end of the row, in the last row past the last byte of the slab, and the first window
    starts at byte 0 -- the loads that the bounds check answers with 0 as a whole and that are fetched again element by element.
    ``shifted``: the same view moved by (+3, -2) voxels in (y, x) under the same output grid, so that windows start before the
    slab.  Every voxel equals the oracle's (the view's own voxel, 0 off the view and where the blending weight rounds to 0)."""
    from multiview_stitcher_amd import _lib

    ndim = len(shape)
    sims, params = grid_case(ndim, dtype, (1,) * ndim, shape, 0, False, seed=5)
    if dtype == np.uint8:
        sims = [s.copy(data=(np.asarray(s.data) >> 4).astype(np.uint8)) for s in sims]
    _, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = union_bb(bbs, params, np.ones(ndim))
    if shifted:
        params[0][ndim - 2:ndim, ndim] = (3.0, -2.0)
    order = 0 if dtype == np.float32 else 1       # (float32 tiles at order 1 go to the row kernels)
    _lib.set_option("no_regions", 1)
    try:
        got, want, _, _ = _fuse_on_column(sims, params, out_bb, interpolation_order=order)
    finally:
        _lib.set_option("no_regions", 0)
    assert got.shape == shape and np.count_nonzero(want) > 0.8 * want.size
    np.testing.assert_array_equal(got, want)


# ---- d. a sole contributor with a ramp weight ----

def test_sole_contributor_with_ramp_weight_is_its_own_value(hip_device):
    """Two uint16 tiles of (40, 72) that share 12 columns, through the column kernel ("no_regions").  Outside the shared columns
    one view alone covers a voxel, and on the rim of the mosaic its blending weight w lies on the cosine ramp, 0 < w < 1: the
    normalised weight is w / w == 1, so the output is that view's voxel itself, not the rounded quotient (w v) / w."""
    from multiview_stitcher_amd import _lib, fusion

    sims, params = grid_case(2, np.uint16, (1, 2), (40, 72), (0, 12), False, seed=2)
    sdims = ["y", "x"]
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = union_bb(bbs, params, np.ones(2))
    want, want_f, dbg = fo.fuse_np(list(views), params, out_bb, full_view_bbs=list(bbs), return_debug=True)
    _lib.set_option("no_regions", 1)
    try:
        _reset_counters()
        got = fusion.fuse_np(list(sims), params, bb_to_dicts(out_bb, sdims), full_view_bbs=[bb_to_dicts(b, sdims) for b in bbs])
        _assert_only("fuse_column_chunks")
    finally:
        _lib.set_option("no_regions", 0)
    got = np.asarray(got)
    assert got.shape == (40, 132)
    # by hand: view 0 holds columns 0..71, view 1 columns 60..131 (identity parameters, unit spacing)
    mosaic = np.zeros((2, 40, 132), np.uint16)
    mosaic[0, :, :72] = views[0]["data"]
    mosaic[1, :, 60:] = views[1]["data"]
    w = dbg["raw_weights"]
    for v, cols in ((0, slice(0, 60)), (1, slice(72, 132))):
        assert not np.any(w[1 - v][:, cols] > 0)
        sole = np.zeros((40, 132), bool)
        sole[:, cols] = True
        ramp = sole & (w[v] > 0) & (w[v] < 1)
        assert ramp.sum() > 1000                                  # the rim is there: rows and columns next to the mosaic's border
        np.testing.assert_array_equal(got[ramp], mosaic[v][ramp])
        np.testing.assert_array_equal(got[sole & (w[v] > 0)], mosaic[v][sole & (w[v] > 0)])
        assert not np.any(got[sole & (w[v] == 0)])                # (where the weight rounds to 0, if anywhere)
    assert_fused_close(got, want, want_f, noise_floor=reference_noise_floor(dbg, want_f))
