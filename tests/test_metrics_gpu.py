"""GPU tests of the registration quality metrics: mvs_pair_moments against the scipy restatement of tests/metrics_oracle.py, the
reduction against the two-pass float64 NCC of the very samples mvs_resample writes, and metrics.tile_pair_image_metrics end to end.

Shapes are the smallest that reach every path: x extents that are a multiple of neither 4 nor 64, halfspaces that cut through the
grid, candidates on both sides of the 8-per-launch group, grids of less than one workgroup, exactly one, several, and more than one
launch covers in a single step of its grid-stride loop."""
import functools

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _metric_ops, metrics, msi_utils, mv_graph
from multiview_stitcher_amd.device import DeviceArray, to_device
from multiview_stitcher_amd.transformation import resample_array
from tests import metrics_oracle as mo
from tests.metrics_helpers import assert_same_structure, make_tile, translation_affine

pytestmark = pytest.mark.gpu

DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
TILE = {3: (11, 20, 37), 2: (33, 41)}


def rotation(ndim, angle, scale):
    """Rotation by ``angle`` in the (y, x) plane times ``scale``."""
    m = np.eye(ndim)
    c, s = np.cos(angle), np.sin(angle)
    m[-2:, -2:] = [[c, -s], [s, c]]
    return m * scale


def about_centre(matrix, shape, shift):
    """(matrix, offset) of index -> matrix @ (index - centre) + centre + shift."""
    ctr = (np.asarray(shape, dtype=float) - 1) / 2
    return matrix, ctr - matrix @ ctr + np.asarray(shift, dtype=float)


def texture(shape, seed, dtype):
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    t = ndimage.gaussian_filter(rng.random(shape), 1.2)
    t = (t - t.min()) / (t.max() - t.min())
    if dtype == np.uint8:
        return (t * 255).astype(np.uint8)
    if dtype == np.uint16:
        return (t * 60000).astype(np.uint16)
    return (t * 3.0 - 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(ndim, dtype_name):
    """Two tiles, the grid, the halfspaces and nine candidates of tests (a) and (b), with the oracle's samples -- built once."""
    dtype = DTYPES[dtype_name]
    shape = TILE[ndim]
    scene = texture(tuple(s + 8 for s in shape), 11 + ndim, dtype)
    fixed = np.ascontiguousarray(scene[tuple(slice(2, 2 + s) for s in shape)])
    moving = np.ascontiguousarray(scene[tuple(slice(5, 5 + s) for s in shape)])
    if dtype == np.float32:
        rng = np.random.default_rng(5)
        for tile in (fixed, moving):                 # a dozen NaN voxels over the two tiles
            for _ in range(6):
                tile[tuple(rng.integers(1, s - 1) for s in shape)] = np.nan
    grid_shape = shape
    fixed_affine = (np.eye(ndim), np.array([0.3, -1.6, 2.45][-ndim:]))          # part of the grid lies outside the fixed tile
    cands = []
    for k in range(9):                               # the moving tile rotated by 0.2 rad and scaled by 0.95, nine nearby poses
        shift = np.array([0.21 * (k % 3) - 0.173, 0.37 * k - 1.1, 2.3 - 0.53 * k])[-ndim:]
        cands.append(about_centre(rotation(ndim, 0.2 + 0.003 * k, 0.95), shape, shift))
    # a rotated box that cuts through the grid: normals at 0.35 rad in the (y, x) plane, and two z planes in 3D
    ctr = (np.asarray(grid_shape, dtype=float) - 1) / 2
    half = 0.43 * np.asarray(grid_shape[-2:], dtype=float)
    rows = []
    for ax, sign in ((0, 1), (0, -1), (1, 1), (1, -1)):
        n2 = sign * rotation(2, 0.35, 1.0)[ax]
        n = np.concatenate([np.zeros(ndim - 2), n2])
        rows.append(np.concatenate([n, [-(n @ ctr) - half[ax] - 0.0137]]))
    if ndim == 3:
        rows.append([1.0, 0.013, -0.007, -(grid_shape[0] - 1.62)])
        rows.append([-1.0, 0.011, 0.009, 0.41])
    halfspaces = np.array(rows)
    want = mo.pair_moments(fixed, moving, fixed_affine, cands, grid_shape, halfspaces)
    return {"fixed": fixed, "moving": moving, "grid_shape": grid_shape, "fixed_affine": fixed_affine, "cands": cands,
            "halfspaces": halfspaces, "want": want}


def assert_inputs_are_off_the_edges(c):
    """The input condition of the exact count: no grid voxel within 1e-9 of a halfspace plane or within 1e-6 px of a tile border."""
    idx = [np.arange(n, dtype=np.float64) for n in c["grid_shape"]]
    assert mo.halfspace_distances(idx, c["halfspaces"]) > 1e-9
    assert mo.sample_border_distance(*c["fixed_affine"], c["grid_shape"], c["fixed"].shape) > 1e-6
    for m, o in c["cands"]:
        assert mo.sample_border_distance(m, o, c["grid_shape"], c["moving"].shape) > 1e-6


def materialised_ncc(fixed, moving, fixed_affine, cand, grid_shape, halfspaces, device):
    """The NCC of the reference's formulation on the device's own samples: mvs_resample of both tiles, the halfspace mask on the
    fixed one, and the host's two-pass float64 sums."""
    f = np.array(resample_array(fixed, fixed_affine[0], fixed_affine[1], grid_shape, order=1, cval=np.nan, device=device, out_on_device=False))
    if halfspaces is not None and len(halfspaces):
        f[~metrics.halfspace_mask(halfspaces, tuple(grid_shape))] = np.nan
    m = np.asarray(resample_array(moving, cand[0], cand[1], grid_shape, order=1, cval=np.nan, device=device, out_on_device=False))
    return metrics.normalized_cross_correlation(f, m)


def assert_paths_agree(got_moments, fixed, moving, fixed_affine, cands, grid_shape, halfspaces, device):
    """Test (b): the same device samples, summed by the kernel and by the host.  Double sums of n <= 1e5 terms differ by at most
    about n 2^-53 ~ 1e-11 relative; 1e-9 absolute is that times 100."""
    for k, cand in enumerate(cands):
        a = _metric_ops.ncc_from_moments(got_moments[k])
        b = materialised_ncc(fixed, moving, fixed_affine, cand, grid_shape, halfspaces, device)
        print(f"candidate {k}: kernel ncc {a!r} materialised {b!r} diff {abs(a - b):.3g}")
        assert np.isnan(a) == np.isnan(b)
        assert np.isnan(a) or abs(a - b) <= 1e-9, (k, a, b)


# ---- (a) moments against the oracle, (b) the two paths ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("ndim", [2, 3])
def test_moments_match_the_oracle(hip_device, ndim, dtype_name):
    c = case(ndim, dtype_name)
    assert_inputs_are_off_the_edges(c)
    assert 0.2 * np.prod(c["grid_shape"]) < c["want"][:, 0].min() and c["want"][:, 0].max() < 0.8 * np.prod(c["grid_shape"])   # masked and out-of-tile regions occur
    scale = float(np.nanmax(np.abs(c["fixed"].astype(np.float64))))
    for K in (1, 3, 9):                              # 9 crosses the 8-per-launch group
        got = _metric_ops.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], c["cands"][:K], c["grid_shape"], c["halfspaces"], hip_device)
        want = c["want"][:K]
        assert got.shape == (K, 6)
        print(f"ndim {ndim} {dtype_name} K {K}: n {got[:, 0]}, max mean diff {np.abs(got[:, 1:3] - want[:, 1:3]).max():.3g}")
        assert np.array_equal(got[:, 0], want[:, 0])
        np.testing.assert_allclose(got[:, 1:3], want[:, 1:3], rtol=1e-5, atol=1e-4 * scale)
        assert np.array_equal(got, _metric_ops.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], c["cands"], c["grid_shape"], c["halfspaces"], hip_device)[:K])


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("ndim", [2, 3])
def test_kernel_and_materialised_paths_agree(hip_device, ndim, dtype_name):
    c = case(ndim, dtype_name)
    got = _metric_ops.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], c["cands"], c["grid_shape"], c["halfspaces"], hip_device)
    assert_paths_agree(got, c["fixed"], c["moving"], c["fixed_affine"], c["cands"], c["grid_shape"], c["halfspaces"], hip_device)


# ---- (c) cancellation ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def camera_case(ndim):
    """16-bit tiles at 60000 +- 3: the same noise in both plus independent noise of sigma 1, 0.37 px apart."""
    shape = TILE[ndim]
    rng = np.random.default_rng(17)
    from scipy import ndimage

    common = ndimage.gaussian_filter(rng.standard_normal(shape), 1.0)
    common /= common.std()
    fixed = (60000 + np.round(3 * common + rng.standard_normal(shape))).astype(np.uint16)
    moving = (60000 + np.round(3 * common + rng.standard_normal(shape))).astype(np.uint16)
    fixed_affine = (np.eye(ndim), np.array([0.0, 1.0, 1.0][-ndim:]))
    cand = (np.eye(ndim), fixed_affine[1] + np.array([0.0, 0.37, 0.37][-ndim:]))
    grid_shape = tuple(s - 3 if k >= ndim - 2 else s for k, s in enumerate(shape))      # every grid voxel lies inside both tiles
    return fixed, moving, fixed_affine, cand, grid_shape


@pytest.mark.parametrize("ndim", [2, 3])
def test_cancellation_on_a_16_bit_camera_offset(hip_device, ndim):
    """Measured on an MI355X: d_ref 3.53e-6 (2D) and 5.37e-6 (3D), the GPU 6.62e-6 and 1.79e-5 from the float32-sample
    oracle, i.e. 1.9 and 3.3 times d_ref against the bound of 8."""
    fixed, moving, fixed_affine, cand, grid_shape = camera_case(ndim)
    assert abs(float(fixed.mean()) - 60000) < 1 and 2.5 < float(fixed.std()) < 4
    got = _metric_ops.pair_moments(fixed, moving, fixed_affine, [cand], grid_shape, None, hip_device)
    assert got[0, 0] == np.prod(grid_shape) and 2.0 ** 2 * got[0, 0] < got[0, 3] < 4.0 ** 2 * got[0, 0]      # the variance survives
    assert_paths_agree(got, fixed, moving, fixed_affine, [cand], grid_shape, None, hip_device)
    ncc32 = _metric_ops.ncc_from_moments(mo.pair_moments(fixed, moving, fixed_affine, [cand], grid_shape, None, sample_dtype=np.float32)[0])
    ncc64 = _metric_ops.ncc_from_moments(mo.pair_moments(fixed, moving, fixed_affine, [cand], grid_shape, None, sample_dtype=np.float64)[0])
    d_ref = abs(ncc32 - ncc64)                       # the reference's own sampling-rounding floor
    bound = 8 * d_ref if d_ref > 0 else 1e-9         # the device rounds at each of seven fma steps where scipy rounds once
    d_gpu = abs(_metric_ops.ncc_from_moments(got[0]) - ncc32)
    print(f"ndim {ndim}: ncc32 {ncc32!r} ncc64 {ncc64!r} d_ref {d_ref:.3g} gpu {_metric_ops.ncc_from_moments(got[0])!r} d_gpu {d_gpu:.3g}")
    assert 0.5 < ncc32 < 0.999
    assert d_gpu <= bound, (d_gpu, d_ref)


# ---- (d) block structure ------------------------------------------------------------------------------------------------------------
B = _lib.MVS_PAIR_BLOCK_VOXELS
BLOCK_GRIDS = {
    "less than one workgroup": (7, 31),                                   # 217 voxels: 1 record
    "exactly one workgroup": (16, B // 16),                              # 1 record
    "three workgroups and five voxels": (1, 3 * B + 5),                  # 4 records
    "more than one step of the launch": (3, _lib.MVS_PAIR_MAX_BLOCKS * B // 2 + 7),   # 2048 records, a second step of the grid-stride loop
}


@pytest.mark.parametrize("name", list(BLOCK_GRIDS))
def test_block_structure(hip_device, name):
    grid_shape = BLOCK_GRIDS[name]
    assert B == 256 and [int(np.ceil(np.prod(g) / B)) for g in list(BLOCK_GRIDS.values())[:3]] == [1, 1, 4]
    assert np.prod(BLOCK_GRIDS["more than one step of the launch"]) > _lib.MVS_PAIR_MAX_BLOCKS * B
    c = case(2, "u16")
    # the grid is laid over the tile's interior at whatever sampling its shape needs
    span = np.asarray(c["fixed"].shape, dtype=float) - 3.0
    step = span / np.maximum(np.asarray(grid_shape, dtype=float) - 1, 1)
    fixed_affine = (np.diag(step), np.array([1.25, 1.5]))
    cands = [(rotation(2, 0.02 * (k + 1), 1.0) @ np.diag(step), np.array([1.7 + 0.3 * k, 1.1])) for k in range(3)]
    # the plane 0.05 y + x = 0.88 span_x of the pixel frame, in grid index coordinates: it cuts the far end of every row off
    halfspaces = np.array([[0.05 * step[0], 1.0 * step[1], -0.88 * span[1] + 0.00123]])
    got = _metric_ops.pair_moments(c["fixed"], c["moving"], fixed_affine, cands, grid_shape, halfspaces, hip_device)
    assert 0 < got[:, 0].min() and got[:, 0].max() < np.prod(grid_shape)
    assert_paths_agree(got, c["fixed"], c["moving"], fixed_affine, cands, grid_shape, halfspaces, hip_device)
    again = _metric_ops.pair_moments(c["fixed"], c["moving"], fixed_affine, cands, grid_shape, halfspaces, hip_device)
    assert got.tobytes() == again.tobytes()


# ---- (e) edge cases -----------------------------------------------------------------------------------------------------------------
def test_no_sample_pairs(hip_device):
    c = case(2, "u8")
    everything_masked = np.array([[0.0, 0.0, 1.0]])
    got = _metric_ops.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], c["cands"][:2], c["grid_shape"], everything_masked, hip_device)
    assert np.array_equal(got, np.zeros((2, 6))) and np.isnan(_metric_ops.ncc_from_moments(got[0]))
    # no halfspaces: every voxel passes the mask; a candidate that maps the moving tile wholly outside has no pair, the other one
    # has one per voxel that lies in both tiles
    far = (np.eye(2), np.array([500.0, -500.0]))
    got = _metric_ops.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], [far, c["cands"][0]], c["grid_shape"], None, hip_device)
    assert np.array_equal(got[0], np.zeros(6)) and np.isnan(_metric_ops.ncc_from_moments(got[0]))
    want = mo.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], [c["cands"][0]], c["grid_shape"], None)
    assert got[1, 0] == want[0, 0] > c["want"][0, 0]


def test_constant_tile_has_zero_variance_exactly(hip_device):
    """Tile origins on the pixel grid: every sample is a tap times 1 plus taps times 0, exact in float32.  (At fractional offsets the
    interpolation of a constant may leave rounding noise where the reference returns NaN -- DESIGN.md -- and is not asserted.)"""
    fixed = np.full((33, 41), 60123, np.uint16)
    moving = case(2, "u16")["moving"]
    got = _metric_ops.pair_moments(fixed, moving, (np.eye(2), np.array([2.0, 3.0])), [(np.eye(2), np.array([1.0, 4.0]))], (30, 36), None, hip_device)
    assert got[0, 0] == 30 * 36 and got[0, 1] == 60123.0 and got[0, 3] == 0.0 and got[0, 5] == 0.0 and got[0, 4] > 0
    assert np.isnan(_metric_ops.ncc_from_moments(got[0]))


@pytest.mark.parametrize("ndim", [2, 3])
def test_host_device_and_strided_views_give_the_same_bits(hip_device, ndim):
    c = case(ndim, "u16")
    args = (c["fixed_affine"], c["cands"][:3], c["grid_shape"], c["halfspaces"], hip_device)
    host = _metric_ops.pair_moments(c["fixed"], c["moving"], *args)
    dev = _metric_ops.pair_moments(DeviceArray.from_host(c["fixed"], hip_device), DeviceArray.from_host(c["moving"], hip_device), *args)
    # windows of larger resident arrays: other strides, a data pointer inside the allocation
    pad = [(2, 1), (3, 2), (5, 4)][-ndim:]
    window = tuple(slice(lo, lo + s) for (lo, _), s in zip(pad, c["fixed"].shape))
    big_f = DeviceArray.from_host(np.pad(c["fixed"], pad, constant_values=7), hip_device)
    big_m = DeviceArray.from_host(np.pad(c["moving"], pad, constant_values=9), hip_device)
    assert not big_f[window].is_contiguous()
    strided = _metric_ops.pair_moments(big_f[window], big_m[window], *args)
    assert host.tobytes() == dev.tobytes() == strided.tobytes()


def test_mixed_dtypes_are_refused(hip_device):
    c8, c16 = case(2, "u8"), case(2, "u16")
    with pytest.raises(_lib.MvsError, match="share one dtype") as e:
        _metric_ops.pair_moments(c8["fixed"], c16["moving"], c8["fixed_affine"], c8["cands"][:1], c8["grid_shape"], None, hip_device)
    assert e.value.code == -4                        # MVS_ERR_UNSUPPORTED


# ---- (f) the public function ------------------------------------------------------------------------------------------------------
def ncc_bounds(views, kwargs):
    """Test (c)'s bound per pair and candidate key: 8 times the difference between the oracle on float64 and on float32 samples,
    the reference's own sampling-rounding floor (1e-9 where there is none)."""
    w64 = mo.tile_pair_image_metrics(views, sample_dtype=np.float64, **kwargs)["pairs"]
    w32 = mo.tile_pair_image_metrics(views, sample_dtype=np.float32, **kwargs)["pairs"]
    out = {}
    for p in w32:
        for q in w32[p]:
            d = abs(w64[p][q]["ncc"] - w32[p][q]["ncc"])
            out[p, q] = 8 * d if d > 0 else 1e-9
    return out


def test_mosaic_of_four_tiles_under_two_keys(hip_device):
    """A 2 x 2 mosaic of 48 x 56 px tiles with 12 px overlaps; key "stage" is right, key "off" has tile 3 off by 1.5 px."""
    scene = texture((100, 120), 23, np.uint16)
    tiles = []
    for i, (y0, x0) in enumerate([(0, 0), (0, 44), (36, 0), (36, 44)]):
        stage = translation_affine((float(y0), float(x0)))
        off = translation_affine((float(y0), x0 + (1.5 if i == 3 else 0.0)))
        tiles.append(make_tile(np.ascontiguousarray(scene[y0:y0 + 48, x0:x0 + 56]), {"stage": stage, "off": off}))
    msims, views = [t[0] for t in tiles], [t[1] for t in tiles]
    mad = lambda a, b: np.nanmean(np.abs(a - b))
    seen = []

    def recording_mad(a, b):
        seen.append((a.copy(), b.copy()))
        return mad(a, b)

    got = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys=["stage", "off"], device=hip_device,
                                          metric_funcs={"ncc": metrics.normalized_cross_correlation, "mad": recording_mad})
    kwargs = dict(base_key="stage", query_keys=["stage", "off"])
    oracle_seen = []

    def oracle_mad(a, b):
        oracle_seen.append((a.copy(), b.copy()))
        return mad(a, b)

    want = mo.tile_pair_image_metrics(views, metric_funcs={"ncc": mo.normalized_cross_correlation, "mad": oracle_mad}, **kwargs)
    assert_same_structure(got, want)
    assert set(got["pairs"]) >= {(0, 1), (0, 2), (1, 3), (2, 3)}
    bounds = ncc_bounds(views, kwargs)
    for p in want["pairs"]:
        for q in ("stage", "off"):
            bound = bounds[p, q]
            diff = abs(got["pairs"][p][q]["ncc"] - want["pairs"][p][q]["ncc"])
            print(f"pair {p} key {q}: ncc {got['pairs'][p][q]['ncc']!r} oracle {want['pairs'][p][q]['ncc']!r} diff {diff:.3g} bound {bound:.3g}")
            assert diff <= bound, (p, q, diff, bound)
    assert got["summary"]["stage"]["ncc"] > got["summary"]["off"]["ncc"]
    for q in ("stage", "off"):                       # a weighted mean of values that are each within their bound
        assert abs(got["summary"][q]["ncc"] - want["summary"][q]["ncc"]) <= max(bounds.values())
    # the custom callable: float32 arrays with NaN exactly where the oracle has them, values within the resample bar
    assert len(seen) == len(oracle_seen) == 2 * len(want["pairs"])
    by_pair = lambda calls, result: {(p, q): calls[2 * i + j] for i, p in enumerate(result["pairs"]) for j, q in enumerate(("stage", "off"))}
    seen, oracle_seen = by_pair(seen, got), by_pair(oracle_seen, want)
    for key, (oa, ob) in oracle_seen.items():
        a, b = seen[key]
        assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == oa.shape
        assert np.array_equal(np.isnan(a), np.isnan(oa)) and np.array_equal(np.isnan(b), np.isnan(ob))
        for x, ox in ((a, oa), (b, ob)):
            ok = ~np.isnan(ox)
            np.testing.assert_allclose(x[ok], ox[ok], rtol=1e-5, atol=1e-4 * float(np.abs(ox[ok]).max()))
    for p in want["pairs"]:
        for q in ("stage", "off"):
            assert got["pairs"][p][q]["mad"] == pytest.approx(want["pairs"][p][q]["mad"], rel=1e-5, abs=1e-4 * 60000)
    # tiles resident on the device are read in place and give the same numbers
    resident = [msi_utils.MultiscaleSpatialImage([to_device(m["scale0"], hip_device)], m.transforms) for m in msims]
    again = metrics.tile_pair_image_metrics(resident, "stage", query_transform_keys=["stage", "off"], device=hip_device)
    for p in want["pairs"]:
        for q in ("stage", "off"):
            assert again["pairs"][p][q]["ncc"] == got["pairs"][p][q]["ncc"]


def test_two_volumes_from_a_pairs_graph_in_both_directions(hip_device):
    """A 2 x 1 x 1 mosaic of (10, 24, 40) volumes that overlap by four planes, Mode 2, bidirectional."""
    scene = texture((16, 24, 40), 29, np.uint16)
    tiles = [make_tile(np.ascontiguousarray(scene[z0:z0 + 10]), {"stage": translation_affine((float(z0), 0.0, 0.0))}) for z0 in (0, 6)]
    msims, views = [t[0] for t in tiles], [t[1] for t in tiles]
    T_edge = translation_affine((0.25, -0.5, 0.75))
    g = mv_graph.Graph([0, 1])
    g.add_edge(0, 1, transform=T_edge)
    got = metrics.tile_pair_image_metrics(msims, "stage", pairs_graph=g, bidirectional=True, device=hip_device)
    kwargs = dict(base_key="stage", pairs_graph={(0, 1): T_edge}, bidirectional=True)
    want = mo.tile_pair_image_metrics(views, **kwargs)
    assert_same_structure(got, want)
    assert list(got["pairs"]) == [(0, 1), (1, 0)]
    bounds = ncc_bounds(views, kwargs)
    for p in want["pairs"]:
        w = want["pairs"][p]["transform"]["ncc"]
        if not np.isnan(w):
            diff, bound = abs(got["pairs"][p]["transform"]["ncc"] - w), bounds[p, "transform"]
            print(f"pair {p}: ncc {got['pairs'][p]['transform']['ncc']!r} oracle {w!r} diff {diff:.3g} bound {bound:.3g}")
            assert diff <= bound, (p, diff, bound)
    assert 0.5 < got["pairs"][(0, 1)]["transform"]["ncc"] < 1.0
