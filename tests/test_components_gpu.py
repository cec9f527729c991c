"""GPU tests of connected-component labelling (labels.label_components, csrc/mvs_components.hip) against scipy.ndimage.label
(tests/components_oracle.py).  The result is an integer image that the restatement defines uniquely, so every comparison is exact
equality.  Masks and shapes: tests/components_cases.py."""
import numpy as np
import pytest
from scipy import ndimage

from multiview_stitcher_amd import _label_ops, labels
from multiview_stitcher_amd.device import DeviceArray, is_device_array
from tests import components_cases as cc
from tests import components_oracle as co
from tests import labels_cases as lc
from tests import labels_oracle as lo

pytestmark = pytest.mark.gpu

DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def given_tile(tile, source, device):
    """``tile`` as the test hands it over: the host array, a resident copy, or a strided window of a larger resident array whose rows
    start three voxels in (off the 16-byte grid), surrounded by foreground that must not leak in."""
    if source == "host":
        return tile
    if source == "device":
        return DeviceArray.from_host(np.ascontiguousarray(tile), device)
    fill = np.iinfo(tile.dtype).max if np.issubdtype(tile.dtype, np.integer) else np.inf
    big = np.full(tuple(n + p for n, p in zip(tile.shape, (2, 5, 9)[3 - tile.ndim:])), fill, dtype=tile.dtype)
    window = tuple(slice(o, o + n) for o, n in zip((1, 2, 3)[3 - tile.ndim:], tile.shape))
    big[window] = tile
    dev = DeviceArray.from_host(big, device)[window]
    assert dev.strides[-1] == 1 and tuple(dev.shape) == tile.shape
    return dev


def run(tile, threshold, connectivity, device, min_voxels=1, out_on_device=False):
    """``(labels as numpy, n, was the result resident)``"""
    got, n = _label_ops.label_components(tile, threshold, connectivity=connectivity, min_voxels=min_voxels, device=device, out_on_device=out_on_device)
    resident = is_device_array(got)
    got = got.get() if resident else got
    assert got.dtype == np.int32
    return got, n, resident


def check(got, n, name, connectivity, min_voxels=1):
    want, want_n = cc.want(name, connectivity, min_voxels)
    assert n == want_n
    assert got.shape == want.shape and np.array_equal(got, want)


# the dtype and the way the tile is handed over change with the case, so that every combination meets small and wide shapes
SOURCES = ["host", "device", "device_window"]
CASES = [(name, list(DTYPES)[i % 3], SOURCES[(i // 3 + i) % 3]) for i, name in enumerate(cc.NAMES)]


@pytest.mark.parametrize("name,dtype,source", CASES, ids=[f"{n}-{d}-{s}" for n, d, s in CASES])
def test_every_case_at_every_connectivity(name, dtype, source, hip_device):
    tile, threshold = cc.as_image(cc.mask(name), DTYPES[dtype])
    for connectivity in cc.connectivities(name):
        got, n, resident = run(given_tile(tile, source, hip_device), threshold, connectivity, hip_device)
        assert resident == (source != "host")
        check(got, n, name, connectivity)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", ["random_2d_50", "random_3d_50", "aligned_256"])
def test_dtypes_and_sources(name, dtype, source, hip_device):
    """uint8 / uint16 / float32 x host array, resident copy, strided resident window; host and device results."""
    tile, threshold = cc.as_image(cc.mask(name), DTYPES[dtype])
    for connectivity in cc.connectivities(name):
        for out_on_device in (False, True):
            got, n, resident = run(given_tile(tile, source, hip_device), threshold, connectivity, hip_device, out_on_device=out_on_device)
            assert resident == (out_on_device or source != "host")
            check(got, n, name, connectivity)


@pytest.mark.parametrize("min_voxels", [2, 5, 10**7])
@pytest.mark.parametrize("name", ["random_2d_50", "random_3d_50", "checkerboard", "volume_40x70x131", "runs_across_ranges"])
def test_min_voxels(name, min_voxels, hip_device):
    tile, threshold = cc.as_image(cc.mask(name), np.uint8)
    for connectivity in cc.connectivities(name):
        got, n, _ = run(tile, threshold, connectivity, hip_device, min_voxels=min_voxels)
        check(got, n, name, connectivity, min_voxels)
        if min_voxels == 10**7:
            assert n == 0 and not got.any()


def test_mask_with_threshold_none_and_min_voxels_below_one(hip_device):
    m = cc.mask("random_2d_50").astype(np.uint8) * 255
    for min_voxels in (1, 0, -3):
        got, n = _label_ops.label_components(m, None, min_voxels=min_voxels, device=hip_device)
        check(got, n, "random_2d_50", 1)


def test_float_tile_with_nans_and_values_equal_to_the_threshold(hip_device):
    tile = cc.float_tile()
    for source in SOURCES:
        for connectivity in (1, 2):
            want, want_n = co.label_components(tile, cc.FLOAT_THRESHOLD, connectivity)
            got, n, _ = run(given_tile(np.array(tile), source, hip_device), cc.FLOAT_THRESHOLD, connectivity, hip_device)
            assert n == want_n and np.array_equal(got, want)
    # a threshold that float32 cannot hold is rounded first: 0.5 + 1e-9 is 0.5
    got, n, _ = run(np.array(tile), cc.FLOAT_THRESHOLD + 1e-9, 1, hip_device)
    want, want_n = co.label_components(tile, cc.FLOAT_THRESHOLD, 1)
    assert n == want_n and np.array_equal(got, want)
    # a negative threshold: the voxels beyond a row's end are still no foreground
    got, n, _ = run(np.zeros((3, 70), np.float32), -1.0, 1, hip_device)
    assert n == 1 and (got == 1).all()


@pytest.mark.parametrize("name", ["comb", "volume_40x70x131", "all_foreground_wide"])
def test_the_same_call_twice_gives_the_same_bits(name, hip_device):
    tile, threshold = cc.as_image(cc.mask(name), np.uint16)
    connectivity = cc.mask(name).ndim
    dev = given_tile(tile, "device", hip_device)
    first = run(dev, threshold, connectivity, hip_device, min_voxels=2)
    second = run(dev, threshold, connectivity, hip_device, min_voxels=2)
    assert first[1] == second[1] and first[0].tobytes() == second[0].tobytes()
    check(first[0], first[1], name, connectivity, 2)


@pytest.mark.parametrize("source", ["host", "device"])
def test_disc_mosaic_from_images_to_one_label_image(source, hip_device):
    """The disc mosaic as uint16 image tiles: label_components per tile, then stitch_labels, equals scipy.ndimage.label of the whole
    mosaic's mask up to a bijection of the ids, which must exist; per tile the labels are the oracle's, with the source's geometry."""
    truth_mask, sims = cc.disc_image_tiles()
    whole, n_whole = ndimage.label(truth_mask)
    given = [s.copy(data=given_tile(np.asarray(s.data), source, hip_device)) for s in sims]
    tiles = labels.label_components(given, cc.DISC_THRESHOLD, device=hip_device)
    for tile, sim in zip(tiles, sims):
        want, want_n = co.label_components(np.asarray(sim.data), cc.DISC_THRESHOLD)
        assert is_device_array(tile.data) == (source == "device") and tile.attrs["n_labels"] == want_n
        assert np.array_equal(tile.data.get() if source == "device" else tile.data, want)
        assert np.array_equal(np.asarray(tile.coords["y"]), np.asarray(sim.coords["y"])) and np.array_equal(np.asarray(tile.coords["x"]), np.asarray(sim.coords["x"]))
    res = labels.stitch_labels(tiles, lc.KEY, device=hip_device)
    assert res.attrs["n_objects"] == n_whole == lc.N_DISCS
    assert res.data.shape == whole.shape and lo.same_up_to_bijection(res.data, whole)
