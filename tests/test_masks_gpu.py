"""GPU tests of the sample masks (masks.py, csrc/mvs_masks.hip) against the numpy / scipy restatement of tests/masks_oracle.py.
Every result is an integer or a selection, so every comparison is exact.

Shapes are the smallest that reach every path: rows that are no multiple of 16 bytes (130, 67, 70 voxels) and tiles of different
shapes, strided device windows whose rows start off the 16-byte grid, a dilation radius wider than one 16-byte lane group that
reaches past the row end, more than 64 views in one brick, label runs that cross a wave's 64 voxels."""
import numpy as np
import pytest

from multiview_stitcher_amd import _detect_ops, _mask_ops, masks, mv_graph, registration
from multiview_stitcher_amd import spatial_image_utils as si
from multiview_stitcher_amd.device import DeviceArray, is_device_array
from tests import masks_oracle as mo

pytestmark = pytest.mark.gpu

KEY = "affine_manual"


# ---- histogram ------------------------------------------------------------------------------------------------------------------------
HIST_SHAPES = [(3, 37, 130), (2, 5, 67)]


def hist_tiles(dtype):
    """Two tiles of different shapes and, for float32, the range the counts are taken over: float32 tiles carry NaNs, values
    exactly on inner edges of both bin counts, on lo and on hi, and values outside the range."""
    rng = np.random.default_rng(11)
    tiles = []
    for shape in HIST_SHAPES:
        if dtype == np.uint8:
            t = rng.integers(0, 256, shape).astype(np.uint8)
        elif dtype == np.uint16:
            t = (rng.gamma(2.0, 3000.0, shape).clip(0, 65535)).astype(np.uint16)
        else:
            t = rng.normal(128.0, 60.0, shape).astype(np.float32)
            flat = t.reshape(-1)
            flat[::17] = np.nan
            flat[5::29] = rng.integers(1, 256, flat[5::29].size)                 # inner edges of 256 bins over [0, 256]
            flat[7::31] = rng.integers(1, 4096, flat[7::31].size) / 16.0         # inner edges of 4096 bins
            flat[3::101] = 0.0                                                   # lo
            flat[4::103] = 256.0                                                 # hi
            flat[9::107] = -3.5                                                  # outside
            flat[10::109] = 300.25
        tiles.append(t)
    return tiles


@pytest.mark.parametrize("n_bins", [256, 4096])
@pytest.mark.parametrize("source", ["host", "device_window"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_histogram_counts_and_range(dtype, source, n_bins, hip_device):
    tiles = hist_tiles(dtype)
    if source == "device_window":
        given = [DeviceArray.from_host(t, hip_device)[:, 1:, 3:] for t in tiles]      # rows start 3 elements off, pitches unchanged
        tiles = [t[:, 1:, 3:] for t in tiles]
        assert not given[0].is_contiguous()
    else:
        given = tiles
    lo, hi, n = _mask_ops.value_range(given, hip_device)
    want_lo, want_hi, want_n = mo.value_range(tiles)
    print(dtype.__name__, source, "range", lo, hi, n)
    assert (lo, hi, n) == (want_lo, want_hi, want_n)
    ranges = [(lo, hi)] + ([(0.0, 256.0)] if dtype == np.float32 else [])
    for r_lo, r_hi in ranges:
        got = _mask_ops.histogram(given, n_bins, r_lo, r_hi, hip_device)
        want, edges = mo.histogram(tiles, n_bins, r_lo, r_hi)
        np.testing.assert_array_equal(_mask_ops.bin_edges(n_bins, r_lo, r_hi), edges)
        assert got.dtype == np.uint64
        np.testing.assert_array_equal(got, want)
        if (r_lo, r_hi) == (0.0, 256.0):
            assert int(got.sum()) < want_n          # NaNs apart, some values lie outside the range


def test_otsu_threshold_is_threshold_otsu_of_all_voxels(hip_device):
    tiles = hist_tiles(np.uint16)
    sims = [si.to_spatial_image(t, dims=["z", "y", "x"], scale=dict(zip("zyx", (1.0, 1.0, 1.0))), translation=dict(zip("zyx", (0.0, 0.0, 0.0)))) for t in tiles]
    want = mv_graph.threshold_otsu(np.concatenate([t.ravel() for t in tiles]))
    assert masks.otsu_threshold(sims, device=hip_device) == want
    values = np.concatenate([t.ravel() for t in tiles]).astype(np.float64)
    counts, _ = np.histogram(values, 1000, (values.min(), values.max()))
    assert masks.otsu_threshold(sims, n_bins=1000, device=hip_device) == mv_graph.otsu_from_histogram(counts, values.min(), values.max())


# ---- threshold and dilation ---------------------------------------------------------------------------------------------------------
def mask_tile(dtype, shape):
    """A sparse tile: set voxels in the first and the last voxel of a row, at two volume corners and at a few seeded places; the
    float32 tile also holds NaNs and the threshold itself (not above it)."""
    rng = np.random.default_rng(5)
    t = np.zeros(shape, dtype=np.float64)
    if dtype == np.float32:
        t.reshape(-1)[3::11] = np.nan
    last = tuple(n - 1 for n in shape)
    mid = tuple(n // 2 for n in shape[:-1])
    for _ in range(6):
        t[tuple(rng.integers(0, n) for n in shape)] = 150.0
    for at in [(0,) * len(shape), last, mid + (0,), mid + (shape[-1] - 1,)]:
        t[at] = 200.0
    t = t.astype(dtype)
    threshold = 100.5
    if dtype == np.float32:
        threshold = 0.1
        t[t == 0] = np.float32(0.1)                 # == (float)threshold: not sample
        t[t > 100] = np.nextafter(np.float32(0.1), np.float32(1.0))      # the smallest float32 above it
    else:
        t[t == 0] = 100                             # below 100.5; 101 and 200 above
        t[t == 150] = 101
    return t, threshold


@pytest.mark.parametrize("radius", [(0, 0, 0), (1, 2, 3), (0, 0, 32)])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_threshold_and_dilation_3d(dtype, radius, hip_device):
    tile, threshold = mask_tile(dtype, (5, 9, 70))
    want = mo.threshold_mask(tile, threshold, radius)
    assert 0 < want.sum() < want.size
    for given in (tile, DeviceArray.from_host(tile, hip_device)):
        got, n_set = _mask_ops.threshold_mask(given, threshold, radius, hip_device)
        assert is_device_array(got) and got.dtype == np.uint8
        np.testing.assert_array_equal(got.get(), want)
        assert n_set == int(want.sum())


def test_threshold_of_a_strided_window_and_2d(hip_device):
    tile, threshold = mask_tile(np.uint16, (9, 70))
    for radius in [(0, 0), (2, 17), (8, 32)]:
        got, n_set = _mask_ops.threshold_mask(tile, threshold, radius, hip_device)
        want = mo.threshold_mask(tile, threshold, radius)
        np.testing.assert_array_equal(got.get(), want)
        assert n_set == int(want.sum())
    big, threshold = mask_tile(np.float32, (5, 9, 70))
    window = DeviceArray.from_host(big, hip_device)[1:, 2:, 5:]
    got, n_set = _mask_ops.threshold_mask(window, threshold, 1, hip_device)
    want = mo.threshold_mask(big[1:, 2:, 5:], threshold, (1, 1, 1))
    np.testing.assert_array_equal(got.get(), want)
    assert n_set == int(want.sum())


# ---- label fuse -----------------------------------------------------------------------------------------------------------------------
def rotation(ndim, angle):
    """Rotation by ``angle``: in the plane (2D), about the axis (1, 1, 1) (3D, so that no axis keeps integer coordinates)."""
    if ndim == 2:
        c, s = np.cos(angle), np.sin(angle)
        return np.array([[c, -s], [s, c]])
    k = np.ones(3) / np.sqrt(3.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def affine_of(linear, shift, centre):
    """x -> linear (x - centre) + centre + shift"""
    n = len(shift)
    a = np.eye(n + 1)
    a[:n, :n] = linear
    a[:n, n] = np.asarray(centre) - linear @ np.asarray(centre) + np.asarray(shift)
    return a


def mask_sim(mask, affine):
    sdims = ["z", "y", "x"][-mask.ndim:]
    sim = si.to_spatial_image(mask, dims=sdims, scale={d: 1.0 for d in sdims}, translation={d: 0.0 for d in sdims})
    si.set_sim_affine(sim, affine, KEY)
    return sim


def three_views(shape):
    """Three masks of one shape: the first rotated by 0.2 rad and placed lowest on every axis (the output origin is then no grid
    point of any view), one under a fractional translation, one further out so that part of the grid stays uncovered."""
    rng = np.random.default_rng(8)
    ndim = len(shape)
    centre = (np.asarray(shape) - 1) / 2.0
    shifts = {2: [(-4.3, -5.2), (3.3, 7.6), (9.45, 21.7)], 3: [(-2.3, -4.3, -5.2), (0.4, 3.3, 7.6), (1.15, 9.45, 21.7)]}[ndim]
    linear = [rotation(ndim, 0.2), np.eye(ndim), np.eye(ndim)]
    masks_ = [(rng.random(shape) < 0.5).astype(np.uint8) for _ in range(3)]
    return masks_, [affine_of(m, s, centre) for m, s in zip(linear, shifts)]


def strip_views(n_views=70, shape=(6, 9)):
    rng = np.random.default_rng(9)
    centre = (np.asarray(shape) - 1) / 2.0
    affines = [affine_of(rotation(2, 0.2), (-2.3, -3.1), centre)]
    affines += [affine_of(np.eye(2), (0.3 + 0.013 * i, 4.37 * i + 0.21), centre) for i in range(1, n_views)]
    return [(rng.random(shape) < 0.6).astype(np.uint8) for _ in range(n_views)], affines


def check_fuse(masks_, affines, hip_device, resident):
    """masks.fuse_labels against the oracle on the grid it chose.  Input condition, asserted: no sampling coordinate lies within
    1e-6 of a half-integer (where order 0 changes voxel) or of a view border (where in-bounds changes)."""
    sims = [mask_sim(DeviceArray.from_host(m, hip_device) if resident else m, a) for m, a in zip(masks_, affines)]
    fused = masks.fuse_labels(sims, KEY, device=hip_device, output_on_backend=resident)
    assert is_device_array(fused.data) == resident and fused.dtype == np.int32 and fused.attrs["n_labels"] == len(masks_)
    sdims = list(fused.dims)
    out_bb = {"origin": si.get_origin_from_sim(fused, asarray=True), "spacing": si.get_spacing_from_sim(fused, asarray=True),
              "shape": np.array(fused.shape)}
    ndim = len(sdims)
    origins, spacings = [np.zeros(ndim)] * len(masks_), [np.ones(ndim)] * len(masks_)
    for m, a in zip(masks_, affines):
        c = mo.sampling_coordinates(a, np.zeros(ndim), np.ones(ndim), out_bb)
        assert np.abs(c - np.floor(c) - 0.5).min() > 1e-6
        for k, n in enumerate(m.shape):
            assert min(np.abs(c[k]).min(), np.abs(c[k] - (n - 1)).min()) > 1e-6
    want = mo.fuse_labels(masks_, affines, origins, spacings, out_bb)
    got = np.asarray(fused.data.get() if resident else fused.data)
    np.testing.assert_array_equal(got, want)
    return want


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("shape", [(20, 33), (5, 20, 33)])
def test_label_fuse_three_views(shape, resident, hip_device):
    masks_, affines = three_views(shape)
    want = check_fuse(masks_, affines, hip_device, resident)
    assert set(np.unique(want)) == {0, 1, 2, 3}


def test_label_fuse_of_70_views(hip_device):
    masks_, affines = strip_views()
    want = check_fuse(masks_, affines, hip_device, False)
    assert want.max() == 70 and len(np.unique(want)) == 71


# ---- contacts -------------------------------------------------------------------------------------------------------------------------
def contact_labels():
    lab = np.zeros((6, 9, 70), np.int32)
    lab[0, 2, 5], lab[0, 3, 4] = 1, 2               # touch only across (0, +1, -1)
    lab[5, 8, 10], lab[5, 8, 11] = 3, 4             # touch only in the last row of the last plane
    lab[2, 2, 20], lab[2, 2, 22] = 5, 6             # background between them: no pair
    lab[3, 3:6, 30:40] = 7                          # touches itself
    z, y, x = np.meshgrid(np.arange(3), np.arange(5, 9), np.arange(70), indexing="ij")
    lab[0:3, 5:9, :] = 8 + ((x // 2 + 7 * z + 3 * y) % 63)      # ids 8 .. 70 in runs of two
    lab[4, 0:2, :], lab[4, 2:4, :] = 20, 21         # a face of 70 voxels: runs that cross a wave's 64
    return lab


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("connectivity", [1, None])
def test_label_contacts(connectivity, resident, hip_device):
    lab = contact_labels()
    assert lab.max() == 70
    given = DeviceArray.empty(lab.shape, np.int32, hip_device) if resident else lab
    if resident:
        given._buf.upload(lab)
    want = mo.contact_counts(lab, 70, connectivity)
    got = _mask_ops.label_contacts(given, 70, connectivity, hip_device)
    np.testing.assert_array_equal(got, want)
    assert got[0, 1] == (0 if connectivity == 1 else 1) and got[2, 3] == 1 and got[4, 5] == 0 and got[19, 20] >= 70
    assert not np.tril(got).any()
    pairs, counts = masks.contact_pairs(given, connectivity=connectivity, return_counts=True, device=hip_device, n_labels=70)
    assert pairs == mo.pairs_of(want) and pairs == sorted(pairs) and all(i < j for i, j in pairs)
    np.testing.assert_array_equal(counts, [want[i, j] for i, j in pairs])
    assert ((0, 1) in pairs) == (connectivity is None) and (2, 3) in pairs and (4, 5) not in pairs
    if not resident:
        np.testing.assert_array_equal(mv_graph.get_connected_labels(lab, np.ones((3, 3, 3)), connectivity=connectivity, device=hip_device),
                                      np.array(pairs).reshape(-1, 2))


def test_label_contacts_2d(hip_device):
    lab = contact_labels()[0]
    for connectivity in (1, 2):
        want = mo.contact_counts(lab, 70, connectivity)
        np.testing.assert_array_equal(_mask_ops.label_contacts(lab, 70, connectivity, hip_device), want)
    assert want[0, 1] == 1


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_end_to_end_pairs_of_a_sparse_row(hip_device):
    sims, _ = mo.sparse_row(KEY)
    threshold = masks.otsu_threshold(sims, device=hip_device)
    assert threshold == mv_graph.threshold_otsu(np.concatenate([np.asarray(s.data).ravel() for s in sims]))
    assert 100 < threshold < 600
    mask_sims = masks.sample_masks(sims, dilate=1, device=hip_device)
    for m, s in zip(mask_sims, sims):
        np.testing.assert_array_equal(m.data, mo.threshold_mask(s.data, threshold, (1, 1)))
        assert m.dtype == np.uint8 and m.dims == s.dims and KEY in m.attrs["transforms"]
        np.testing.assert_array_equal(m.coords["x"], s.coords["x"])
    assert [bool(m.data.any()) for m in mask_sims] == [True, True, False, True]
    pairs, fused = registration.get_pairs_from_sample_masks(mask_sims, transform_key=KEY, device=hip_device)
    assert pairs == [(0, 1)]
    assert fused.shape == (64, 208) and set(np.unique(fused.data)) == {0, 1, 2, 4}
    params = registration.register(sims, transform_key=KEY, new_transform_key="reg", pairs=pairs, pre_registration_pruning_method=None,
                                   device=hip_device)
    assert len(params) == 4
    shift = np.asarray(si.get_affine_from_sim(sims[1], "reg"))[:2, 2] - np.asarray(si.get_affine_from_sim(sims[0], "reg"))[:2, 2]
    assert np.abs(shift).max() < 0.5            # the tiles were cut from one scene at their stage positions


def test_sample_masks_of_binned_smoothed_resident_tiles(hip_device):
    """Binning, smoothing, threshold and dilation in order, on resident tiles; the masks sit on the binned coordinates."""
    sims, _ = mo.sparse_row(KEY)
    resident = [s.copy(data=DeviceArray.from_host(s.data, hip_device)) for s in sims]
    binning, sigma = {"y": 2, "x": 2}, 1.0
    got = masks.sample_masks(resident, binning=binning, sigma=sigma, dilate={"x": 2}, device=hip_device, keep_on_device=True)
    conditioned = [_detect_ops.gaussian_smooth(registration._bin_sim(s, binning, hip_device).data, [sigma, sigma], hip_device) for s in resident]
    lo, hi, _ = _mask_ops.value_range(conditioned, hip_device)
    values = np.concatenate([c.get().ravel() for c in conditioned]).astype(np.float64)
    assert (lo, hi) == (values.min(), values.max())
    threshold = masks.otsu_threshold(resident, binning=binning, sigma=sigma, device=hip_device)
    assert threshold == mv_graph.threshold_otsu(values)
    for m, s, c in zip(got, sims, conditioned):
        assert is_device_array(m.data) and m.shape == (32, 32)
        np.testing.assert_array_equal(m.coords["x"], registration._binned_coords(np.asarray(s.coords["x"]), 2))
        np.testing.assert_array_equal(m.coords["y"], registration._binned_coords(np.asarray(s.coords["y"]), 2))
        np.testing.assert_array_equal(m.data.get(), mo.threshold_mask(c.get(), threshold, (0, 2)))
    pairs, _ = registration.get_pairs_from_sample_masks(got, transform_key=KEY, device=hip_device)
    assert pairs == [(0, 1)]
