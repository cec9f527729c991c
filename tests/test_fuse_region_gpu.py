"""GPU parity of the REGION kernels of mvs_fuse_chunk (copy_region_kernel / fuse_region_kernel<1, 2, 4, 8> /
fuse_region_mixed_kernel in csrc/mvs_fuse_region.hip) against the oracle's fuse_np, one case per path.

The region kernels fuse every weighted-average chunk of translated tiles that the planner (csrc/mvs_region_plan.h) accepts: the
fuse hot path.  The regular grids of test_fuse_gpu.py show them identity or all-fractional parameters only; here every case is
built for one path -- the 512-voxel copy bricks and their raw tail stores, whole-pixel offsets of a registered mosaic (border
clustering, "partial" views, the per-brick ``covered`` refinement, the lean plain-mean path, the ``anchored`` / ``plain``
shortcuts), 3 and 5..8 views on a cell, the brick widths at their limits, a sole contributor on its ramp, the fork onto side
streams, the plan cache.  All cases run with DEFAULT options unless they say otherwise.  Every case resets the counters
"fuse_*_chunks" and asserts afterwards that the region kernels fused the chunk and no other family ran, reads
"fuse_class_out_vox_<k>" (k = 0 one-view rim boxes, 1 two views, 2 three / four views, 3 five to eight views, 4 copy) and asserts
that the classes it was built for are there, and proves on the oracle's debug output (``raw_weights``, ``views``) that the voxels
it exists for are there in quantity.

Data: independent white noise per view over the whole range of the dtype (tests.helpers.placed_tiles): two views on one voxel
differ by about a third of the range, so a blend weight that is wrong by 1e-3 moves a uint16 output by about 20 counts (the
smoothed mosaics of the other files: 0.3), and the top bits of uint16 pass through the pack / unpack code of Row8 / store8.
Bars: the defaults of ``assert_fused_close`` with the oracle's float result and ``reference_noise_floor``; ``assert_array_equal``
where one view decides a voxel; bitwise equality between two option settings of this library."""
import numpy as np
import pytest

from oracle import fuse_oracle as fo
from tests.helpers import (assert_fused_close, bb_to_dicts, grid_origins, placed_tiles, reference_noise_floor, shift_params,
                           sim_to_view, stair_tiles, union_bb, white_noise)

pytestmark = pytest.mark.gpu

FAMILIES = ("fuse_rows_chunks", "fuse_region_chunks", "fuse_column_chunks", "fuse_generic_chunks")


def _reset_counters():
    from multiview_stitcher_amd import _lib

    for key in FAMILIES:
        _lib.get_counter(key, reset=True)


def _assert_only_regions():
    """The chunk(s) since the last reset were fused by the region kernels and by nothing else."""
    from multiview_stitcher_amd import _lib

    counts = {key: _lib.get_counter(key, reset=True) for key in FAMILIES}
    assert counts["fuse_region_chunks"] >= 1 and all(v == 0 for k, v in counts.items() if k != "fuse_region_chunks"), counts


def _class_voxels():
    from multiview_stitcher_amd import _lib

    return [_lib.get_counter(f"fuse_class_out_vox_{k}") for k in range(5)]


def _out_bb(sims, params):
    _, bbs = zip(*[sim_to_view(s) for s in sims])
    return union_bb(bbs, params, np.ones(len(bbs[0]["shape"])))


def _oracle(sims, params, out_bb, order=1):
    """(want, want_float, debug, noise floor) of the chunk; ``n_views`` = finite (in-bounds, not NaN) views per voxel."""
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    want, want_f, dbg = fo.fuse_np(list(views), params, out_bb, full_view_bbs=list(bbs), return_debug=True, interpolation_order=order)
    dbg["n_views"] = np.isfinite(dbg["views"]).sum(0)
    return want, want_f, dbg, reference_noise_floor(dbg, want_f)


def _fuse(sims, params, out_bb, order=1, classes=(), **options):
    """fusion.fuse_np under ``options`` with the counters around it: the region kernels fused the chunk, no other family ran, and
    the ``classes`` the case was built for hold voxels.  Returns (fused array, voxels per class)."""
    from multiview_stitcher_amd import _lib, fusion
    from multiview_stitcher_amd import spatial_image_utils as si

    sdims = si.get_spatial_dims_from_sim(sims[0])
    _, bbs = zip(*[sim_to_view(s) for s in sims])
    for key, value in options.items():
        _lib.set_option(key, value)
    try:
        _reset_counters()
        got = fusion.fuse_np(list(sims), params, bb_to_dicts(out_bb, sdims), full_view_bbs=[bb_to_dicts(b, sdims) for b in bbs],
                             interpolation_order=order)
        got = np.asarray(got)
        _assert_only_regions()
        vox = _class_voxels()
    finally:
        for key in options:
            _lib.set_option(key, 0)
    assert sum(vox) == got.size, vox
    assert all(vox[k] > 0 for k in classes), vox
    return got, vox


def _parity(sims, params, out_bb=None, order=1, classes=(), **options):
    """One chunk through the oracle and the region kernels under the project's bar: (got, want, debug, voxels per class)."""
    out_bb = out_bb if out_bb is not None else _out_bb(sims, params)
    want, want_f, dbg, floor = _oracle(sims, params, out_bb, order)
    got, vox = _fuse(sims, params, out_bb, order, classes, **options)
    assert_fused_close(got, want, want_f, noise_floor=floor)
    return got, want, dbg, vox


def _order(dtype):
    return 0 if dtype == np.float32 else 1        # (float32 tiles at order 1 go to the row kernels)


# ---- a. copy class, 512-voxel bricks ----

@pytest.mark.parametrize("dtype,t", [(np.uint16, t) for t in range(1, 8)] + [(np.uint8, 3), (np.uint8, 6), (np.float32, 3), (np.float32, 6)])
def test_copy_class_wide_bricks_every_tail(hip_device, dtype, t):
    """One view of (37, 528 + t) voxels on its own grid.  The planner cuts a 4-voxel shell off every border, but on a tile this
    small the weight profile stays above 3e-4 even in the corners (about 0.4 / 529), so every box is one full positive view: the
    whole chunk is copy class.  The interior box and the shell rows above and below it are 520 + t > 160 voxels wide: ``lxb = 6``
    (``copy_brick_item``, the ``lxb >= 4`` branch: ``load_nt``, eight row groups requested back to back, the loaded dwords stored
    as they are by ``store8_bits``).  The second 512-voxel brick of every row holds 8 + t voxels: lane 1 stores a tail of t
    elements -- 4 + 2 + 1 for uint16, byte by byte for uint8; float32 takes the decode / nan_to_num / ``store8`` branch.  29
    interior rows: the 32 rows of a brick are ragged.  One view decides every voxel: exact."""
    sims = placed_tiles(dtype, (37, 528 + t), [(0, 0)], seed=t)
    params = shift_params(2, n=1)
    got, want, dbg, vox = _parity(sims, params, order=_order(dtype), classes=(4,))
    assert dbg["n_views"].min() == 1 and vox[4] == got.size
    assert np.count_nonzero(want) > 0.8 * want.size
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("move", ["none", "whole", "fractional"])
@pytest.mark.parametrize("shape", [(37, 533), (21, 37, 540)])
def test_copy_class_slab_ends_and_tap_planes(hip_device, shape, move):
    """uint16.  ``none``: the view on its own grid; in 3-D the 13 interior planes end in a ragged brick of one plane.  ``whole``:
    the view moved by (+3, -2) voxels in (y, x) under the unchanged output grid: the windows of the first rows start before the
    slab (negative offsets), those of the last lanes run past it: the ``ends`` test of ``copy_brick_item`` sends those row groups
    through decode and the element-wise refetch ``row8_refetch`` (in 3-D the eight corner boxes, whose weight profile falls below
    3e-4, are class 0: ``region_brick<1>``).  ``fractional``: the view moved by fractions of a voxel: ``copy_brick_item`` takes its
    ``anyfrac`` branch (in 3-D five tap planes per brick of four, ``np < 4`` in the last brick; two tap rows and the ninth
    element of every window).  Whole-pixel moves are exact."""
    ndim = len(shape)
    sims = placed_tiles(np.uint16, shape, [(0,) * ndim], seed=3)
    params = shift_params(ndim, n=1)
    out_bb = _out_bb(sims, params)
    if move == "whole":
        params[0][ndim - 2:ndim, ndim] = (3.0, -2.0)
    if move == "fractional":
        params[0][:ndim, ndim] = (0.375, 0.25, -0.625)[3 - ndim:]
    got, want, dbg, vox = _parity(sims, params, out_bb, classes=(4, 0) if ndim == 3 else (4,))
    assert vox[4] > 0.6 * got.size                       # the copy class holds most of the chunk
    assert np.count_nonzero(want) > 0.6 * want.size
    if move != "fractional":
        np.testing.assert_array_equal(got, want)


# ---- b. registered grids: whole-pixel offsets ----

def _registered_grid(ndim, dtype, seed=0):
    tiles, shape, overlap = (((2, 3), (72, 200), (20, 50)) if ndim == 2 else ((2, 2, 2), (24, 40, 72), (8, 12, 20)))
    sims = placed_tiles(dtype, shape, grid_origins(tiles, shape, overlap), seed=seed)
    rng = np.random.default_rng(seed + 17)
    return sims, shift_params(ndim, [rng.integers(-3, 4, ndim).astype(float) for _ in sims])


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_registered_grid_whole_pixel_offsets(hip_device, ndim, dtype):
    """2 x 3 tiles of (72, 200) / 2 x 2 x 2 tiles of (24, 40, 72), every one moved by whole pixels from integers(-3, 4): the
    borders of a grid row lie a few pixels apart, ``axis_breakpoints`` clusters them (``tol = 16``), and the slivers between the
    clustered borders fall into the overlap cells, whose views are flagged "partial" (bits 16-31 of ``allone_mask``).  In
    ``region_brick`` that is the ``covered`` refinement per brick, the per-voxel ``inb`` test, ``allint`` next to a partial view
    (the batched loads of NV = 4), the lean ``region_brick_avg`` on covered unit bricks and the ``anchored`` / ``plain`` shortcut
    with its ``partial && !inb[j]`` zeroing; in 3-D the 8-view corners run NV = 8 with record set B (views 6, 7).  Precondition:
    voxels that fewer views reach than their cell lists -- view counts an exact grid does not have (3 in 2-D; 3, 5, 6, 7 in 3-D).
    Option "fuse_mixed" (one launch over the padded per-XCD list) gives the same bits."""
    sims, params = _registered_grid(ndim, dtype)
    out_bb = _out_bb(sims, params)
    got, want, dbg, vox = _parity(sims, params, out_bb, classes=(4, 1, 2) if ndim == 2 else (4, 1, 2, 3))
    nv = dbg["n_views"]
    odd = np.isin(nv, (3,) if ndim == 2 else (3, 5, 6, 7))
    assert odd.sum() >= (20 if ndim == 2 else 200), odd.sum()
    assert (nv == (4 if ndim == 2 else 8)).sum() >= (500 if ndim == 2 else 150)      # (3-D: at least (8 - 6) (12 - 6) (20 - 6) = 168)
    mixed, _ = _fuse(sims, params, out_bb, fuse_mixed=1)
    np.testing.assert_array_equal(mixed, got)


# ---- c. the clustering limit ----

def test_clustering_limit_16_joins_17_does_not(hip_device):
    """Three uint16 tiles of (48, 120) in a row along x that share 30 columns, at y = 0, 16 and 17.  The lower y borders 0 and 16
    join one cluster (break point 0), 17 does not: tile 1 is "partial" over 16 rows of every cell it shares with tile 0 (bricks
    that the ``covered`` test cannot release: the sliver lies inside them), tile 2 starts a cell of its own.  Precondition: in
    the columns that two tiles share, at least 16 x 30 voxels with ONE view (the sliver rows above tile 1)."""
    sims = placed_tiles(np.uint16, (48, 120), [(0, 0), (16, 90), (17, 180)], seed=4)
    params = shift_params(2, n=3)
    got, want, dbg, vox = _parity(sims, params, classes=(4, 1))
    nv = dbg["n_views"]
    assert got.shape == (65, 300)
    assert (nv[:16, 90:120] == 1).all() and (nv[16:48, 90:120] == 2).all() and (nv[17:64, 180:210] == 2).all()
    np.testing.assert_array_equal(got[:16, 90:120], want[:16, 90:120])          # one view decides these voxels


def test_clustering_along_z_partial_views(hip_device):
    """Three uint16 tiles of (12, 40, 72) in a row along x that share 20 columns, at z = 0, 2 and 5: all z borders cluster (0, 2,
    5 -> 0; 12, 14, 17 -> 17), so every view is partial along z in every cell: the ``zy_ok`` half of the per-voxel bounds test,
    and bricks of 4 planes of which the view covers some.  Precondition: overlap columns hold planes with one and with two views."""
    sims = placed_tiles(np.uint16, (12, 40, 72), [(0, 0, 0), (2, 0, 52), (5, 0, 104)], seed=5)
    params = shift_params(3, n=3)
    got, want, dbg, vox = _parity(sims, params, classes=(1,))
    nv = dbg["n_views"]
    assert got.shape == (17, 40, 176)
    assert (nv[:, :, 52:72] == 1).sum() >= 1000 and (nv[:, :, 52:72] == 2).sum() >= 1000 and (nv == 0).sum() >= 1000
    assert not got[nv == 0].any()


# ---- d. stairs: 1..8 views on a cell ----

STAIR_WIDE = ((136, 168), (18, 20))          # steps above tol = 16: no clustering, cells of 1..n views, all of them full
STAIR_CLUSTERED = ((64, 96), (6, 9))         # steps below it: clustered borders, partial views in the NV = 4 and NV = 8 bodies


def _stair(n, geometry, dtype, fractional, seed=0):
    shape, step = geometry
    sims = stair_tiles(dtype, shape, n, step, seed=seed)
    rng = np.random.default_rng(seed + 29)
    # (fractions below half a voxel: the borders of the wide stair stay more than 16 voxels apart)
    shifts = [rng.uniform(-0.45, 0.45, 2) for _ in sims] if fractional else None
    return sims, shift_params(2, shifts, n=n)


@pytest.mark.parametrize("fractional", [False, True])
@pytest.mark.parametrize("geometry", [STAIR_WIDE, STAIR_CLUSTERED], ids=["wide", "clustered"])
@pytest.mark.parametrize("n", [7, 8])
def test_stairs_of_7_and_8_views(hip_device, n, geometry, fractional):
    """uint16 stairs, tile i at i * step.  Wide: cells of 1, 2, ... n views: three views in the NV = 4 instantiation (the padded
    ``vv = v < nv ? v : 0`` lanes of ``region_brick_avg`` and the ``v < nv`` guards of ``region_brick``), five to eight views in
    the NV = 8 instantiation, whose views 6 and 7 come from record set B (``R.b`` in ``rec_field``).  Clustered: the same bodies
    with partial views.  Whole-pixel parameters take the single-tap rows (``allint``, batched loads), fractional ones the four
    tap rows of ``fetch_val``.  Precondition: at least 1000 voxels (clustered stair: 100) with exactly 3, 5, 6 and 7 finite views
    each; the 8-view cell of the wide stair is (136 - 7 * 18) x (168 - 7 * 20) = 280 voxels, less a row and a column when shifted."""
    sims, params = _stair(n, geometry, np.uint16, fractional, seed=n)
    got, want, dbg, vox = _parity(sims, params, classes=(2, 3))
    nv = dbg["n_views"]
    for k in (3, 5, 6, 7) + ((8,) if n == 8 else ()):
        assert (nv == k).sum() >= (100 if geometry is STAIR_CLUSTERED else 243 if k == 8 else 1000), (k, (nv == k).sum())


def test_stair_of_8_views_uint8(hip_device):
    """The wide stair of 8 views on uint8 tiles: ``Row8<unsigned char>`` (8-byte windows, byte unpack) in the NV = 4 / 8 bodies."""
    sims, params = _stair(8, STAIR_WIDE, np.uint8, False, seed=3)
    got, want, dbg, vox = _parity(sims, params, classes=(2, 3))
    assert (dbg["n_views"] == 8).sum() == 280 and (dbg["n_views"] == 7).sum() >= 1000


@pytest.mark.parametrize("geometry", [STAIR_WIDE, STAIR_CLUSTERED], ids=["wide", "clustered"])
def test_stair_of_8_views_float32_order0_drops_nan(hip_device, geometry):
    """float32 tiles at order 0 with 60 NaN voxels sprinkled over every view: float tiles never take the lean or the ``plain``
    path (``ISF``); a NaN drops its view from that voxel (``val[j] == val[j]``), a voxel whose views are all NaN comes out 0.
    The one-view cells of a stair are thin copy-class boxes (``lxb = 1``, the last branch of ``copy_brick_item``): they must read
    their one tap only -- a NaN at (y + 1, x + 1) under a zero interpolation weight once turned the voxels (y, x), (y, x + 1) and
    (y + 1, x) into 0 (89 voxels of the wide stair)."""
    sims, params = _stair(8, geometry, np.float32, False, seed=6)
    rng = np.random.default_rng(12)
    for i, s in enumerate(sims):
        d = np.array(s.data, dtype=np.float32, copy=True)
        d[tuple(rng.integers(0, n, 60) for n in d.shape)] = np.nan
        sims[i] = s.copy(data=d)
    got, want, dbg, vox = _parity(sims, params, order=0, classes=(2, 3))
    assert np.isfinite(got).all()
    assert (dbg["n_views"] == 7).sum() >= 100            # voxels of the 8-view cells that lost a view to a NaN, among others


# ---- e. brick widths ----

@pytest.mark.parametrize("fractional", [False, True])
@pytest.mark.parametrize("W", [9, 32, 33, 136, 137, 300, 600])
def test_two_tiles_sharing_W_columns(hip_device, W, fractional):
    """Two uint16 tiles of (37, W + 140) that share W columns: the overlap box is W wide -- ``lxb = 1`` up to 32, 3 from 33 to 136,
    4 from 137 (9: the borders cluster, 16-voxel bricks with partial views).  Fractional: the second tile moved by (0.25, 0.5).
    W = 300 and 600 have 80 rows: at least 1000 overlap voxels where both raw weights are exactly 1 (the ``unit`` accumulation
    and the per-lane ``lane_unit`` test).  At W = 300 every 128-voxel brick of the overlap still holds a ramp end of one tile (a
    ramp is about (W + 141) / 4 voxels long); at W = 600 the brick [396, 524) x [36, 68) lies off every ramp: both views unit on a
    whole brick, the lean ``region_brick_avg`` of NV = 2 (whole-pixel offsets)."""
    rows = 80 if W >= 300 else 37
    sims = placed_tiles(np.uint16, (rows, W + 140), [(0, 0), (0, 140)], seed=W)
    params = shift_params(2, [(0.0, 0.0), (0.25, 0.5) if fractional else (0.0, 0.0)])
    got, want, dbg, vox = _parity(sims, params, classes=(4, 1))
    both = (dbg["n_views"] == 2)
    assert both.sum() >= (rows - 1) * (W - 1)
    if W >= 300:
        w = dbg["raw_weights"]
        unit = both & (w[0] == 1) & (w[1] == 1)
        assert unit.sum() >= 1000
        assert W < 600 or unit[36:68, 396:524].all()           # the brick of the lean path


@pytest.mark.parametrize("W", [33, 137])
def test_two_tiles_sharing_W_columns_3d(hip_device, W):
    """The 3-D pair of (6, 37, W + 140) tiles: six planes, a brick of four and a ragged one of two, in 64- and 128-voxel bricks."""
    sims = placed_tiles(np.uint16, (6, 37, W + 140), [(0, 0, 0), (0, 0, 140)], seed=W)
    got, want, dbg, vox = _parity(sims, shift_params(3, n=2), classes=(1,))
    assert (dbg["n_views"] == 2).sum() == 6 * 37 * W


def test_two_tiles_stacked_along_z(hip_device):
    """Two uint16 tiles of (24, 40, 72) that share 16 planes: the overlap is a slab of whole rows, its interior (off the y / x
    shells and the z ramps) the plain mean of two full rows."""
    sims = placed_tiles(np.uint16, (24, 40, 72), [(0, 0, 0), (8, 0, 0)], seed=8)
    got, want, dbg, vox = _parity(sims, shift_params(3, n=2), classes=(1,))
    assert got.shape == (32, 40, 72) and (dbg["n_views"] == 2).sum() == 16 * 40 * 72


# ---- f. a sole contributor on the ramp ----

@pytest.mark.parametrize("shape", [(40, 72), (12, 5400)])
def test_sole_contributor_with_ramp_weight_is_its_own_value(hip_device, shape):
    """Two uint16 tiles that share 12 columns, default options (the column file's case d on the region kernels).  Outside the
    shared columns one view alone covers a voxel, and on the rim of the mosaic its blending weight w lies on the cosine ramp,
    0 < w < 1: the output must be the view's own voxel, not the rounded quotient (w v) / w.  (40, 72): the weight profile stays
    above 3e-4 up to the corners (0.4 / 73), so the planner puts the rim into the copy class.  (12, 5400): near the corners the
    profile falls to 0.1 / 5401 < 3e-4 and the ramp weight rounds to 0 there -- the corner boxes are class 0 (``region_brick<1>``:
    the ``nv == 1`` threshold 3e-4 of ``need`` / ``lane_unit``, else the ``last`` / ``wlast`` bookkeeping of the general
    accumulation); where the weight is 0 the output is 0."""
    ny, nx = shape
    sims = placed_tiles(np.uint16, shape, [(0, 0), (0, nx - 12)], seed=2)
    params = shift_params(2, n=2)
    got, want, dbg, vox = _parity(sims, params, classes=(1, 4) if nx < 1000 else (0, 1, 4))
    assert got.shape == (ny, 2 * nx - 12)
    mosaic = np.zeros((2,) + got.shape, np.uint16)
    mosaic[0, :, :nx] = np.asarray(sims[0].data)
    mosaic[1, :, nx - 12:] = np.asarray(sims[1].data)
    w = dbg["raw_weights"]
    for v, cols in ((0, slice(0, nx - 12)), (1, slice(nx, 2 * nx - 12))):
        assert not np.any(w[1 - v][:, cols] > 0)
        sole = np.zeros(got.shape, bool)
        sole[:, cols] = True
        ramp = sole & (w[v] > 0) & (w[v] < 1)
        assert ramp.sum() > 1000                                  # the rim is there: rows and columns next to the mosaic's border
        np.testing.assert_array_equal(got[ramp], mosaic[v][ramp])
        np.testing.assert_array_equal(got[sole & (w[v] > 0)], mosaic[v][sole & (w[v] > 0)])
        if nx > 1000:
            assert (sole & (w[v] == 0)).sum() >= 2 and mosaic[v][sole & (w[v] == 0)].any()      # the weight does round to 0
        assert not np.any(got[sole & (w[v] == 0)])


# ---- g. the fork onto the side streams ----

def test_forked_launch_equals_serial_classes(hip_device):
    """A 3-D stair of 5 uint16 views of (92, 92, 92), step 17: 160^3 voxels in 4096 bricks or more, the size from which the class
    kernels run side by side -- NV = 2 on the main stream, the others on side streams between the fork and join events.  With
    option "serial_classes" the same launch stays on one stream.  Same bits, both within the oracle's bar."""
    from multiview_stitcher_amd import _lib

    sims = stair_tiles(np.uint16, (92, 92, 92), 5, (17, 17, 17), seed=9)
    params = shift_params(3, n=5)
    out_bb = _out_bb(sims, params)
    want, want_f, dbg, floor = _oracle(sims, params, out_bb)
    assert want.shape == (160, 160, 160) and (dbg["n_views"] == 5).sum() >= 1000
    forked, vox = _fuse(sims, params, out_bb, classes=(0, 1, 2, 3, 4))
    assert _lib.get_counter("fuse_region_bricks") >= 4096 and _lib.get_counter("fuse_region_forked") == 1
    serial, _ = _fuse(sims, params, out_bb, serial_classes=1)
    assert _lib.get_counter("fuse_region_bricks") >= 4096 and _lib.get_counter("fuse_region_forked") == 0
    np.testing.assert_array_equal(forked, serial)
    assert_fused_close(forked, want, want_f, noise_floor=floor)
    assert_fused_close(serial, want, want_f, noise_floor=floor)


# ---- h. the plan cache ----

def test_plan_cache_follows_the_geometry_not_the_data(hip_device):
    """Device-resident uint16 tiles (the same slabs in every call).  Geometry A (two tiles sharing 33 columns), A again, geometry B
    (the second tile moved by 5 rows), then A with new data in the same slabs: "fuse_plan_ms" is 0 exactly when the geometry of
    the call before is repeated (the plan is still on the device), positive after a change; every result is its oracle's."""
    from multiview_stitcher_amd import _lib
    from multiview_stitcher_amd.device import DeviceArray, to_device

    host = placed_tiles(np.uint16, (37, 173), [(0, 0), (0, 140)], seed=10)
    sims = [to_device(s, 0) for s in host]
    geo_a = shift_params(2, n=2)
    geo_b = shift_params(2, [(0.0, 0.0), (5.0, 0.0)])
    out_bb = _out_bb(host, geo_b)            # one output grid for both geometries

    def run(current, params):
        want, want_f, dbg, floor = _oracle(current, params, out_bb)
        got, vox = _fuse(sims, params, out_bb, classes=(4, 1))
        plan_ms = _lib.get_counter("fuse_plan_ms")
        assert_fused_close(got, want, want_f, noise_floor=floor)
        return got, plan_ms

    first, ms = run(host, geo_a)
    assert ms > 0
    again, ms = run(host, geo_a)
    assert ms == 0
    np.testing.assert_array_equal(again, first)
    moved, ms = run(host, geo_b)
    assert ms > 0 and not np.array_equal(moved, first)
    rng = np.random.default_rng(11)
    fresh = []
    for s, h in zip(sims, host):
        data = white_noise(rng, h.shape, np.uint16)
        DeviceArray.from_host(data, 0).copy_into(s.data, (0, 0))
        fresh.append(h.copy(data=data))
    _lib.synchronize(0)
    renewed, ms = run(fresh, geo_a)
    assert ms > 0 and not np.array_equal(renewed, first)
    _, ms = run(fresh, geo_a)
    assert ms == 0
