"""GPU: the capped grid-stride launches past their first trip.

Every kernel here runs ``for (i = first; i < items; i += gridDim.x * per_block)`` under a fixed cap of workgroups.  The suites of
their modules use the smallest shapes that reach every path, none of which fills a cap once; here each launch gets a shape of 2.2
to 2.5 trips (tests/launch_caps.py; 1.22 for the mask passes), so that the stride, the barrier at the top of a second step, the
LDS rows a second step writes again and the wave-wide votes inside the loop all run -- against the same oracles and with the same
bars as the module suites.  tests/test_launch_caps_host.py ties the shapes to the caps in the sources.

What makes a skipped or doubled trip visible: inputs are random (not periodic in the trip length); every case asserts on the
reference alone that the items beyond the first trip carry part of the result; outputs that the wrapper lets the caller provide are
pre-filled with values the expected result does not hold; integer results and selections are compared exactly."""
import functools

import numpy as np
import pytest
from scipy import ndimage

from tests import launch_caps as lc

pytestmark = pytest.mark.gpu


def first_trip(name):
    """Items of the first trip of a row of the table."""
    r = lc.row(name)
    return r["cap"] * r["per_block"]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- histogram and range ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hist_tiles(dtype_name):
    """Two tiles of lc.HIST_SHAPES, as hist_tiles of tests/test_masks_gpu.py: float32 tiles carry NaNs, values exactly on inner edges
    of both bin counts, on lo and hi of the range (0, 256) and outside it.  The largest value sits in a row of the second trip and
    the smallest in the very last row (third trip), both inside the device windows [:, 1:, 3:]."""
    rng = np.random.default_rng(31)
    tiles = []
    for shape in lc.HIST_SHAPES:
        if dtype_name == "uint16":
            t = (rng.gamma(2.0, 3000.0, shape).clip(5, 60000)).astype(np.uint16)
        else:
            t = rng.normal(128.0, 60.0, shape).astype(np.float32)
            flat = t.reshape(-1)
            flat[::17] = np.nan
            flat[5::29] = rng.integers(1, 256, flat[5::29].size)
            flat[7::31] = rng.integers(1, 4096, flat[7::31].size) / 16.0
            flat[3::101] = 0.0
            flat[4::103] = 256.0
            flat[9::107] = -3.5
            flat[10::109] = 300.25
        tiles.append(t)
    tiles[0][0, 8500, 10] = 65000 if dtype_name == "uint16" else 9000.25
    tiles[1][-1, -1, -1] = 1 if dtype_name == "uint16" else -1000.5
    return frozen(*tiles)


@pytest.mark.parametrize("source", ["host", "device_window"])
@pytest.mark.parametrize("dtype_name", ["uint16", "float32"])
def test_histogram_and_range_past_the_first_trip(hip_device, dtype_name, source):
    from multiview_stitcher_amd import _mask_ops
    from multiview_stitcher_amd.device import DeviceArray
    from tests import masks_oracle as mo

    tiles = list(hist_tiles(dtype_name))
    if source == "device_window":
        given = [DeviceArray.from_host(t, hip_device)[:, 1:, 3:] for t in tiles]
        tiles = [t[:, 1:, 3:] for t in tiles]
        assert not given[0].is_contiguous() and [t.shape for t in tiles] == lc.HIST_WINDOW_SHAPES
    else:
        given = tiles
    # reference alone: the rows of the first trip hold neither extreme and at most 60 % of the voxels
    n_first = first_trip("masks histogram and range")
    head = tiles[0].reshape(-1, tiles[0].shape[-1])[:n_first]
    want_lo, want_hi, want_n = mo.value_range(tiles)
    assert np.nanmin(head) > want_lo and np.nanmax(head) < want_hi and np.count_nonzero(~np.isnan(head.astype(np.float64))) < 0.6 * want_n
    lo, hi, n = _mask_ops.value_range(given, hip_device)
    print(dtype_name, source, "range", lo, hi, n)
    assert (lo, hi, n) == (want_lo, want_hi, want_n)
    ranges = [(lo, hi)] + ([(0.0, 256.0)] if dtype_name == "float32" else [])
    for r_lo, r_hi in ranges:
        for n_bins in (256, 4096):
            got = _mask_ops.histogram(given, n_bins, r_lo, r_hi, hip_device)
            want, _ = mo.histogram(tiles, n_bins, r_lo, r_hi)
            want_head, _ = mo.histogram([head], n_bins, r_lo, r_hi)
            assert 0 < int(want_head.sum()) < 0.6 * int(want.sum())
            assert got.dtype == np.uint64
            np.testing.assert_array_equal(got, want)


# ---- threshold and dilation ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_tile(dtype_name):
    """A sparse random tile of lc.MASK_SHAPE (4 set voxels in 1000, the first and the last voxel set), in the values of mask_tile of
    tests/test_masks_gpu.py: uint8 100 / 101 / 200 around the threshold 100.5; float32 the threshold itself, the next float32
    above it, and NaNs."""
    rng = np.random.default_rng(32)
    shape = lc.MASK_SHAPE
    level = rng.random(shape)
    level[0, 0, 0] = level[-1, -1, -1] = 0.0
    if dtype_name == "uint8":
        t = np.full(shape, 100, np.uint8)
        t[level < 0.004] = 101
        t[level < 0.001] = 200
        return frozen(t), 100.5
    t = np.full(shape, np.float32(0.1), np.float32)
    t[level < 0.004] = np.nextafter(np.float32(0.1), np.float32(1.0))
    t[(level > 0.5) & (level < 0.6)] = np.nan
    return frozen(t), 0.1


@pytest.mark.parametrize("dtype_name,radius", [("uint8", (0, 0, 0)), ("uint8", (1, 2, 3)), ("uint8", (0, 0, 17)), ("float32", (1, 2, 3))])
def test_threshold_and_dilation_past_the_first_trip(hip_device, dtype_name, radius):
    """(0, 0, 0): the threshold kernel reports n_set; (1, 2, 3): x, y, z passes, the lines kernel last; (0, 0, 17): the x pass last,
    with a radius beyond one 16-voxel group."""
    from multiview_stitcher_amd import _mask_ops
    from multiview_stitcher_amd.device import is_device_array
    from tests import masks_oracle as mo

    tile, threshold = mask_tile(dtype_name)
    want = mo.threshold_mask(tile, threshold, radius)
    # reference alone: the groups beyond the first trip hold set and unset voxels
    groups = -(-tile.shape[-1] // 16)
    tail = want.reshape(-1, tile.shape[-1])[first_trip("masks threshold and dilation") // groups:]
    assert len(tail) > 50000 and 0 < int(tail.sum()) < tail.size and want[-1, -1, -1] == 1
    got, n_set = _mask_ops.threshold_mask(tile, threshold, radius, hip_device)
    assert is_device_array(got) and got.dtype == np.uint8
    print(dtype_name, radius, "n_set", n_set, "of", want.size, "-- beyond the first trip", int(tail.sum()))
    assert n_set == int(want.sum())
    np.testing.assert_array_equal(got.get(), want)


# ---- contacts -----------------------------------------------------------------------------------------------------------------------
N_CONTACT_LABELS = 74


@functools.lru_cache(maxsize=None)
def contact_labels():
    """Labels of lc.CONTACT_SHAPE in the manner of contact_labels of tests/test_masks_gpu.py: random ids 8 .. 70 in runs of two
    voxels on a background of 0, a face of 70 voxels between 20 and 21 (runs that cross a wave's 64 lanes), the pair (71, 72) only
    in the first item of the second trip, the pair (73, 74) only in the last chunk of the last row."""
    rng = np.random.default_rng(33)
    nz, ny, nx = lc.CONTACT_SHAPE
    ids = np.where(rng.random((nz, ny, nx // 2)) < 0.3, rng.integers(8, 71, (nz, ny, nx // 2)), 0)
    lab = np.repeat(ids, 2, axis=2).astype(np.int32)
    lab[1, 100:104, :] = 0
    lab[1, 100:102, :], lab[1, 102:104, :] = 20, 21
    chunks = -(-nx // 64)
    item = first_trip("masks label contacts")                   # the first item of trip 2: a chunk 0
    assert item % chunks == 0
    row = item // chunks
    z, y = divmod(row, ny)
    assert z == 0 and 0 < y < ny - 1
    lab[:, y - 1:y + 2, 0:4] = 0
    lab[z, y, 0], lab[z, y, 1] = 71, 72
    lab[:, ny - 2:, 64:] = 0
    lab[nz - 1, ny - 1, nx - 2], lab[nz - 1, ny - 1, nx - 1] = 73, 74
    return frozen(lab)


@pytest.mark.parametrize("connectivity", [1, None])
def test_label_contacts_past_the_first_trip(hip_device, connectivity):
    from multiview_stitcher_amd import _mask_ops
    from tests import masks_oracle as mo

    lab = contact_labels()
    assert lab.max() == N_CONTACT_LABELS
    want = mo.contact_counts(lab, N_CONTACT_LABELS, connectivity)
    # reference alone: both planted pairs are counted once and touch nothing else; the rows of the first trip hold a part only
    rows_first = first_trip("masks label contacts") // 2
    want_head = mo.contact_counts(lab.reshape(-1, lab.shape[-1])[:rows_first], N_CONTACT_LABELS, 1)
    assert want[70, 71] == 1 and want[72, 73] == 1 and want[70:, :].sum() == 2 and want[:, 70:].sum() == 2
    assert want[19, 20] >= 70 and int(want.sum()) > 2 * int(want_head.sum()) > 0
    got = _mask_ops.label_contacts(lab, N_CONTACT_LABELS, connectivity, hip_device)
    print("connectivity", connectivity, "contacts", int(want.sum()), "pairs", int(np.count_nonzero(want)))
    np.testing.assert_array_equal(got, want)


# ---- local maxima ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plateaus(shape):
    """Integer plateaus 0 .. 5 as _plateaus of tests/test_detection_gpu.py (ties everywhere, exact in float32: no tie margin to keep),
    with one peak of 7 in the first tile of the second trip and one in the very last tile."""
    r = np.random.default_rng(sum(shape)).integers(0, 6, shape).astype(np.float32)
    per_row = -(-shape[-1] // 256)
    row = first_trip("detection local maxima") // per_row
    first = np.unravel_index(row, shape[:-1]) + (3,)
    last = tuple(n - 1 for n in shape[:-1]) + (shape[-1] - 2,)
    r[first] = r[last] = 7.0
    return frozen(r), first, last


@pytest.mark.parametrize("rule", ["plain", "neighbourhood_minimum"])
@pytest.mark.parametrize("shape,window", lc.MAXIMA_CASES, ids=lambda v: "x".join(map(str, v)))
def test_local_maxima_past_the_first_trip(hip_device, shape, window, rule):
    from multiview_stitcher_amd import _detect_ops
    from multiview_stitcher_amd.device import DeviceArray
    from tests import detection_oracle as do

    r, first, last = plateaus(shape)
    sample, bound, size = None, None, None
    if rule == "neighbourhood_minimum":
        size = 3
        sample = np.random.default_rng(1 + sum(shape)).integers(0, 50, shape).astype(np.uint16)
        sample[first] = sample[last] = 0                                # both planted peaks pass the rule
        plain = do.detections(r, window, 0.0)
        bound = float(np.median(ndimage.minimum_filter(sample, size=size, mode="reflect")[plain])) + 0.5
        mask = do.detections(r, window, 0.0, sample, bound, size)
        assert 0 < mask.sum() < plain.sum()
    else:
        mask = do.detections(r, window, 0.0)
    want = np.argwhere(mask)
    # reference alone: detections in the first tile of trip 2 and in the last tile, and most of them beyond the first trip
    per_row = -(-shape[-1] // 256)
    tile_of = np.ravel_multi_index(tuple(want[:, :-1].T), shape[:-1]) * per_row + want[:, -1] // 256
    assert mask[first] and mask[last] and np.count_nonzero(tile_of >= first_trip("detection local maxima")) > len(want) // 2
    dr = DeviceArray.from_host(r, hip_device)
    ds = None if sample is None else DeviceArray.from_host(sample, hip_device)
    sw = None if sample is None else (size,) * len(shape)
    got = _detect_ops.local_maxima(dr, window, 0.0, ds, sw, bound, device=hip_device, capacity=len(want) + 7)
    print(shape, rule, "detections", len(want))
    np.testing.assert_array_equal(got, want)
    if rule == "plain":                                                 # a list that overflows on the way: the count is still exact
        again = _detect_ops.local_maxima(dr, window, 0.0, device=hip_device, capacity=len(want) // 3)
        np.testing.assert_array_equal(again, want)


# ---- field warp and intensity apply -------------------------------------------------------------------------------------------------
WARP_DTYPES = {(150000, 20): np.uint16, (40, 3800, 18): np.uint8}


def far_from(want, dtype):
    """An array of ``dtype`` that differs from ``want`` in every voxel by far more than any bar (half the range of an integer
    type; 1000 for float32, NaN where want is NaN ... replaced by 0)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.nan_to_num(want.astype(np.float32) + np.float32(1000.0), nan=-1000.0).astype(np.float32)
    half = (int(np.iinfo(dtype).max) + 1) // 2
    return ((want.astype(np.int64) + half) % (2 * half)).astype(dtype)


@functools.lru_cache(maxsize=None)
def warp_case(shape, nodes):
    from tests import nonrigid_oracle as no
    from tests.intensity_helpers import texture
    from tests.test_nonrigid_gpu import warp_field_of

    x = texture(shape, 61 + len(shape), WARP_DTYPES[shape])
    field = warp_field_of(nodes, 7)
    return frozen(x, field, no.warp_float(x, field))


@pytest.mark.parametrize("shape,nodes", lc.APPLY_CASES, ids=lambda v: "x".join(map(str, v)))
def test_field_warp_past_the_first_trip(hip_device, shape, nodes):
    from multiview_stitcher_amd import _nonrigid_ops
    from multiview_stitcher_amd.device import DeviceArray
    from tests import nonrigid_oracle as no
    from tests.test_nonrigid_gpu import assert_warp_close

    x, field, want_float = warp_case(shape, nodes)
    # reference alone: the rows beyond the first trip are no copy of the input and not constant
    rows_first = first_trip("non-rigid field warp")
    tail = want_float.reshape(-1, shape[-1])[rows_first:]
    assert len(tail) > rows_first and np.ptp(tail) > 0.5 * np.ptp(want_float)
    assert np.abs(tail - x.reshape(-1, shape[-1])[rows_first:]).max() > 0.1 * np.ptp(want_float)
    dx = DeviceArray.from_host(x, hip_device)
    for out_dtype in dict.fromkeys([x.dtype.type, np.float32]):
        fill = far_from(no.to_dtype(want_float, out_dtype), out_dtype)
        out = DeviceArray.from_host(fill, hip_device)
        got = _nonrigid_ops.warp_field(dx, field, out=out, out_dtype=out_dtype, device=hip_device)
        assert got is out
        assert_warp_close(got.get(), want_float, x, out_dtype)


@functools.lru_cache(maxsize=None)
def apply_case(shape, cells):
    from tests.helpers import apply_coeff, apply_input

    dtype = WARP_DTYPES[shape]
    return frozen(apply_input(shape, dtype, 5), apply_coeff(cells, dtype, 6))


@pytest.mark.parametrize("shape,cells", lc.APPLY_CASES, ids=lambda v: "x".join(map(str, v)))
def test_intensity_apply_past_the_first_trip(hip_device, shape, cells):
    """The bar of test_apply_matches_the_float32_restatement: the bits of the float32 restatement."""
    from multiview_stitcher_amd import _intensity_ops
    from multiview_stitcher_amd.device import DeviceArray
    from tests import intensity_oracle as io
    from tests.helpers import same_bits

    x, coeff = apply_case(shape, cells)
    dx = DeviceArray.from_host(x, hip_device)
    rows_first = first_trip("intensity apply")
    for out_dtype in dict.fromkeys([x.dtype.type, np.float32]):
        want = io.apply(x, coeff, out_dtype)
        tail = want.reshape(-1, shape[-1])[rows_first:]
        assert len(tail) > rows_first and len(np.unique(tail)) > 100        # reference alone: the later trips write varied values
        if np.dtype(out_dtype).kind != "f":
            hi = np.iinfo(out_dtype).max
            assert (tail == 0).any() and (tail == hi).any()
        out = DeviceArray.from_host(far_from(want, out_dtype), hip_device)
        got = _intensity_ops.apply_map(dx, coeff, out=out, out_dtype=out_dtype, device=hip_device)
        assert got is out
        g = got.get()
        print(shape, np.dtype(out_dtype).name, "voxels that differ:", int(np.count_nonzero(g.view(np.uint8) != want.view(np.uint8))))
        assert same_bits(g, want), np.argwhere(g != want)[:5]


# ---- intensity cell moments ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cell_case(cells):
    """Two uint16 tiles cut from one scene and a grid of lc.CELL_GRID that lies inside both.  cells (1, 1, 1): sub-pixel shifts only
    and no halfspace, so that the one record holds every grid voxel.  Other cells: the moving tile also turned by one degree, and
    a halfspace that cuts the grid."""
    from tests import intensity_oracle as io
    from tests.intensity_helpers import rotation, texture

    grid = lc.CELL_GRID
    shape = tuple(g + m for g, m in zip(grid, (2, 4, 8)))
    scene = texture(tuple(s + 8 for s in shape), 24, np.uint16)
    fixed = np.ascontiguousarray(scene[tuple(slice(2, 2 + s) for s in shape)])
    moving = np.ascontiguousarray(scene[tuple(slice(4, 4 + s) for s in shape)])
    fixed_affine = (np.eye(3), np.array([0.3137, 1.2713, 1.4519]))
    shift = np.array([0.1731, 1.6177, 2.2893])
    halfspaces = None
    if cells == (1, 1, 1):
        moving_affine = (np.eye(3), fixed_affine[1] + shift)
    else:
        rot = rotation(3, np.deg2rad(1.0))
        ctr = (np.asarray(grid, dtype=float) - 1) / 2
        moving_affine = (rot, ctr - rot @ ctr + fixed_affine[1] + shift)
        n = np.concatenate([[0.0], rotation(2, 0.35)[1]])
        halfspaces = np.array([np.concatenate([n, [-(n @ ctr) - 0.31 * grid[2] - 0.0137]])])
    c = {"fixed": fixed, "moving": moving, "grid_shape": grid, "fixed_affine": fixed_affine, "moving_affine": moving_affine,
         "halfspaces": halfspaces, "cells_f": cells, "cells_m": cells}
    want = io.cell_pair_moments(fixed, moving, fixed_affine, moving_affine, grid, cells, cells, halfspaces)
    return c, want


@pytest.mark.parametrize("cells", [(1, 1, 1), (2, 1, 2)], ids=lambda v: "x".join(map(str, v)))
def test_intensity_cell_moments_past_the_first_trip(hip_device, cells):
    """The bars of test_moments_match_the_oracle (tests/test_intensity_gpu.py): n exact, the other five to rtol 1e-5 and
    atol 1e-4 max |fixed| -- a bound on float32 samples, not on the length of the double sums."""
    from multiview_stitcher_amd import _intensity_ops, _lib, intensity
    from tests import intensity_oracle as io
    from tests import metrics_oracle as mo

    c, want = cell_case(cells)
    grid = c["grid_shape"]
    assert io.edge_clearance(c["fixed"], c["moving"], c["fixed_affine"], c["moving_affine"], grid, cells, cells) > 1e-6
    if c["halfspaces"] is not None:
        assert mo.halfspace_distances([np.arange(n, dtype=np.float64) for n in grid], c["halfspaces"]) > 1e-9
    records = intensity.plan_records(c["fixed_affine"], c["moving_affine"], grid, c["fixed"].shape, c["moving"].shape, cells, cells)
    keys = [(tuple(r[2]), tuple(r[3])) for r in records]
    blocks = [min(-(-int(np.prod(r[1])) // _lib.MVS_INTENSITY_BLOCK_VOXELS), _lib.MVS_INTENSITY_MAX_BLOCKS) for r in records]
    assert set(want) <= set(keys)
    if cells == (1, 1, 1):
        # reference alone: one record of the whole grid, 2.3 trips of its 1024 workgroups, and every voxel is counted
        assert len(records) == 1 and int(np.prod(records[0][1])) == np.prod(grid) == lc.row("intensity cell moments")["cases"][0][2]
        assert want[keys[0]][0] == np.prod(grid)
    else:
        # records of different workgroup counts share the launch; the later ones hold samples
        assert len(records) >= 4 and len(set(blocks)) >= 2 and sum(1 for k in keys[1:] if k in want and want[k][0] > 1000) >= 3
    got = _intensity_ops.cell_pair_moments(c["fixed"], c["moving"], c["fixed_affine"], c["moving_affine"], cells, cells, records, c["halfspaces"],
                                           device=hip_device)
    atol = 1e-4 * float(np.abs(c["fixed"].astype(np.float64)).max())
    for key, row, nb in zip(keys, got, blocks):
        w = want.get(key, np.zeros(6))
        rel = np.abs(row[1:] - w[1:]) / (atol + 1e-5 * np.abs(w[1:]))
        print(key, "workgroups", nb, "n", row[0], "of", w[0], "max err / bar", rel.max())
        assert row[0] == w[0], (key, row[0], w[0])
        np.testing.assert_allclose(row[1:], w[1:], rtol=1e-5, atol=atol, err_msg=str(key))


# ---- pair moments ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_case(dtype_name):
    """case() of tests/test_metrics_gpu.py on the grid lc.PAIR_GRID: part of the grid outside the fixed tile, five turned and scaled
    candidates, NaN voxels in float32 tiles, and one halfspace through the grid."""
    from tests import metrics_oracle as mo
    from tests.test_metrics_gpu import DTYPES, about_centre, rotation, texture

    dtype = DTYPES[dtype_name]
    shape = lc.PAIR_GRID
    scene = texture(tuple(s + 8 for s in shape), 14, dtype)
    fixed = np.ascontiguousarray(scene[tuple(slice(2, 2 + s) for s in shape)])
    moving = np.ascontiguousarray(scene[tuple(slice(5, 5 + s) for s in shape)])
    if dtype == np.float32:
        rng = np.random.default_rng(5)
        for tile in (fixed, moving):
            for _ in range(200):
                tile[tuple(rng.integers(1, s - 1) for s in shape)] = np.nan
    fixed_affine = (np.eye(3), np.array([0.3, -1.6, 2.45]))
    cands = []
    for k in range(5):
        shift = np.array([0.21 * (k % 3) - 0.173, 0.37 * k - 1.1, 2.3 - 0.53 * k])
        cands.append(about_centre(rotation(3, 0.05 + 0.003 * k, 0.97), shape, shift))
    ctr = (np.asarray(shape, dtype=float) - 1) / 2
    n = np.concatenate([[0.013], rotation(2, 0.35, 1.0)[1]])
    halfspaces = np.array([np.concatenate([n, [-(n @ ctr) - 0.27 * shape[2] - 0.0137]])])
    want = mo.pair_moments(fixed, moving, fixed_affine, cands, shape, halfspaces)
    # the same over the planes that lie wholly beyond the first trip (grid index z >= z0)
    z0 = -(-first_trip("pair moments") // (shape[1] * shape[2]))
    hs_tail = halfspaces.copy()
    hs_tail[:, -1] += hs_tail[:, 0] * z0
    tail_affine = (fixed_affine[0], fixed_affine[1] + fixed_affine[0][:, 0] * z0)
    cand_tail = (cands[0][0], cands[0][1] + cands[0][0][:, 0] * z0)
    want_tail = mo.pair_moments(fixed, moving, tail_affine, [cand_tail], (shape[0] - z0,) + shape[1:], hs_tail)
    return {"fixed": fixed, "moving": moving, "grid_shape": shape, "fixed_affine": fixed_affine, "cands": cands, "halfspaces": halfspaces,
            "want": want, "want_tail": want_tail}


@pytest.mark.parametrize("dtype_name", ["u16", "f32"])
def test_pair_moments_past_the_first_trip(hip_device, dtype_name):
    """The bars of test_moments_match_the_oracle (tests/test_metrics_gpu.py): n exact, the means to rtol 1e-5 and atol 1e-4 of the
    largest value -- a bound on float32 samples, not on the length of the double sums."""
    from multiview_stitcher_amd import _metric_ops
    from tests.test_metrics_gpu import assert_inputs_are_off_the_edges

    c = pair_case(dtype_name)
    assert_inputs_are_off_the_edges(c)
    total = float(np.prod(c["grid_shape"]))
    # reference alone: the halfspace and the tile borders cut samples away, and the planes beyond the first trip hold a large part
    assert 0.2 * total < c["want"][:, 0].min() and c["want"][:, 0].max() < 0.9 * total
    assert 0.3 * c["want"][0, 0] < c["want_tail"][0, 0] < c["want"][0, 0]
    scale = float(np.nanmax(np.abs(c["fixed"].astype(np.float64))))
    for K in (1, 5):                                                    # kernels K = 1 and K = 8
        got = _metric_ops.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], c["cands"][:K], c["grid_shape"], c["halfspaces"], hip_device)
        want = c["want"][:K]
        assert got.shape == (K, 6)
        err = np.abs(got[:, 1:3] - want[:, 1:3])
        print(f"{dtype_name} K {K}: n {got[:, 0]}, max mean err / bar {(err / (1e-4 * scale + 1e-5 * np.abs(want[:, 1:3]))).max():.3g}")
        assert np.array_equal(got[:, 0], want[:, 0])
        np.testing.assert_allclose(got[:, 1:3], want[:, 1:3], rtol=1e-5, atol=1e-4 * scale)


# ---- finite range ---------------------------------------------------------------------------------------------------------------------
def test_finite_range_past_the_first_trip(hip_device):
    from multiview_stitcher_amd import _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    rng = np.random.default_rng(36)
    a = rng.normal(10.0, 50.0, lc.RANGE_N).astype(np.float32)
    a[::13] = np.nan
    a[5::1001] = np.inf
    a[7::1003] = -np.inf
    a[700_000] = 4321.5                                                 # the maximum: in the first trip
    a[lc.RANGE_N - 500] = -8765.25                                      # the minimum: among the last 1000 values
    finite = a[np.isfinite(a)]
    n_first = first_trip("finite range")
    assert finite.max() == a[700_000] and finite.min() == a[-500] and np.nanmin(np.where(np.isfinite(a[:n_first]), a[:n_first], np.nan)) > -1000
    want = (float(finite.min()), float(finite.max()), int(finite.size))
    assert _reg_ops.finite_range(a, hip_device) == want
    assert _reg_ops.finite_range(DeviceArray.from_host(a, hip_device), hip_device) == want


# ---- DCT weights ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dct_case(shape, sharp, blur, seed, patch):
    """pair() of tests/dct_oracle.py -- two views of one random base, blurred differently, so that no block ties in quality -- but
    in random patches of ``patch`` voxels a side the views change roles, so that the better view, and with it the weights, change
    from block to block."""
    rng = np.random.default_rng(seed)
    base = rng.random(shape)
    a = ((ndimage.gaussian_filter(base, sharp) if sharp else base) * 1000 + 100).astype(np.float32)
    b = (ndimage.gaussian_filter(base, blur) * 1000 + 100).astype(np.float32)
    swap = np.kron(rng.random(tuple(-(-s // patch) for s in shape)) < 0.5, np.ones((patch, patch), bool))[:shape[0], :shape[1]]
    return frozen(np.stack([np.where(swap, b, a), np.where(swap, a, b)]))


def check_dct(views, kw, hip_device, general):
    """The bars of test_standalone_weights_match_reference: qualities to 1e-5 of their largest, weights to 1e-5."""
    from multiview_stitcher_amd import _lib, weights
    from tests import dct_oracle as do

    want_q = do.quality_maps(views, **kw)
    want_w = do.content_based_dct(views, **kw)
    _lib.set_option("dct_general", 1 if general else 0, hip_device)
    try:
        w, q = weights.content_based_dct(views, device=hip_device, return_quality=True, **kw)
    finally:
        _lib.set_option("dct_general", 0, hip_device)
    scale = max(float(np.nanmax(np.abs(want_q))), 1e-30)
    assert q.shape == want_q.shape and w.dtype == np.float32 and w.shape == views.shape
    print(f"    {views.shape} {kw} general={general}: quality err / bar {np.nanmax(np.abs(q - want_q)) / (1e-5 * scale):.3g}, "
          f"weight err / bar {np.nanmax(np.abs(w - want_w)) / 1e-5:.3g}")
    np.testing.assert_allclose(q, want_q, rtol=0, atol=1e-5 * scale, equal_nan=True)
    np.testing.assert_allclose(w, want_w, rtol=0, atol=1e-5, equal_nan=True)
    return want_q, want_w


def test_dct_interpolation_past_the_first_trip(hip_device):
    views = dct_case(lc.ELEMENTWISE_SHAPE, 0.7, 2.5, 37, 32)
    _, want_w = check_dct(views, {}, hip_device, False)
    # reference alone: the voxels beyond the first trip carry weights of both kinds, not one value
    tail = want_w.reshape(2, -1)[:, first_trip("DCT weight interpolation"):]
    assert tail.shape[1] > first_trip("DCT weight interpolation") and tail[0].min() < 0.2 and tail[0].max() > 0.8 and len(np.unique(tail[0])) > 1000


def test_dct_general_quality_reuses_its_slots(hip_device):
    views = dct_case(lc.DCT_GENERAL_SHAPE, 0.0, 1.0, 38, 2)
    want_q, _ = check_dct(views, {"dct_size": lc.DCT_GENERAL_SIZE}, hip_device, True)
    # reference alone: the (view, block) items beyond the first trip -- all of view 1 among them -- hold distinct qualities
    tail = want_q.reshape(-1)[first_trip("DCT general quality"):]
    assert want_q.size == lc.row("DCT general quality")["cases"][0][2] and len(tail) > first_trip("DCT general quality")
    assert len(np.unique(tail)) > 1000 and np.all(tail > 0)


@pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("shape,dct_size", [((70, 45), {"y": 40, "x": 33}), ((65, 33), 32)], ids=["70x45-40x33", "65x33-32"])
def test_dct_block_extents_at_and_above_the_lds_limit(hip_device, shape, dct_size, general):
    """Not trips but the block loops next to them: extents 40 and 33 lie above the LDS limit of 32, so the general kernel runs
    without the option (edge blocks of 30 and 12); (65, 33) at 32 has blocks of exactly the limit and far-edge blocks of extent 1
    on both axes, on the LDS path and on the general one."""
    views = dct_case(shape, 0.7, 2.5, 39, 16)
    want_q, _ = check_dct(views, {"dct_size": dct_size}, hip_device, general)
    assert want_q.shape == ((2, 2, 2) if shape == (70, 45) else (2, 3, 2))


# ---- deconvolution --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deconv_case():
    """Two high-frequency views of lc.ELEMENTWISE_SHAPE with holes no view covers (tests/deconv_oracle.py), one iteration -- the
    fewest that runs the update kernels; tests/test_mv_deconv_gpu.py has cases of one -- and one step of boundary erosion, so that
    the coverage and erosion kernels run too."""
    from tests import deconv_oracle as do

    views, blend = do._hf_views(40, 2, lc.ELEMENTWISE_SHAPE, holes=True)
    kw = dict(sample_boundary_erosion_px=1)
    want = do.deconvolve(views, blend, n_iterations=1, **kw)
    return frozen(views, blend, want) + (kw,)


def test_deconvolution_past_the_first_trip(hip_device):
    """The bar of tests/test_mv_deconv_gpu.py: 2e-4 of the largest value, and the zeros of the eroded coverage exactly."""
    from multiview_stitcher_amd import fusion

    views, blend, want, kw = deconv_case()
    n_first = first_trip("deconvolution element-wise")
    tail = want.reshape(-1)[n_first:]
    assert len(tail) > n_first and (tail == 0).any() and np.ptp(tail) > 0.5 * np.ptp(want)      # reference alone
    got = fusion.multi_view_deconvolution(views, blend, n_iterations=1, device=hip_device, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"deconvolution {views.shape}: err {err:.3g}, bar {2e-4 * scale:.3g}")
    np.testing.assert_array_equal(got == 0, want == 0)
    assert err <= 2e-4 * scale
