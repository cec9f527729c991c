"""GPU: ``masks.feather`` (csrc/mvs_mask_feather.hip) against its scipy oracle (tests/mask_feather_oracle.py), byte for byte.

The kernel computes the squared distance exactly in integers; only the last step -- sqrt and cosine in float64 -- could differ from
numpy's in the last ulp.  So every case first asserts, ON THE ORACLE ALONE, that no value before rounding lies within 1e-9 of a
half-integer, and then demands equal bytes.  Shapes (tests/mask_feather_cases.py) are the smallest that reach every path: rows
that are no multiple of the 16-voxel groups, rows of 64 / 65 / 127 voxels at the edges of the x pass's bit window, windows wider
than their axis, an axis of one voxel, 2-D masks, strided device windows whose rows start off the 16-byte grid, z slabs forced
through the library option."""
import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _mask_ops, masks
from multiview_stitcher_amd import spatial_image_utils as si
from multiview_stitcher_amd.device import DeviceArray, is_device_array
from tests import mask_feather_cases as fc
from tests import mask_feather_oracle as fo

pytestmark = pytest.mark.gpu


def oracle(mask, width):
    """The oracle's bytes, after the precondition that makes byte equality a fair demand."""
    before = fo.feather_float(mask, width)
    assert fo.half_integer_distance(before) > 1e-9
    return np.rint(before).astype(np.uint8)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_feather_equals_the_oracle(name, source, hip_device):
    shape, width = fc.CASES[name]
    mask = np.array(fc.blob_mask(shape))
    want = oracle(mask, width)
    assert 0 < (want == 0).sum() < want.size and ((want > 0) & (want < 252)).any()
    given = DeviceArray.from_host(mask, hip_device) if source == "device" else mask
    got = masks.feather(given, width, device=hip_device, keep_on_device=source == "device")
    assert is_device_array(got) == (source == "device")
    got = got.get() if is_device_array(got) else got
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])


def test_zeros_only_in_the_first_plane_and_the_last_column(hip_device):
    mask = fc.first_plane_last_column((9, 7, 45))
    width = (4, 3, 20)
    want = oracle(mask, width)
    assert want[-1, 3, 0] == 252 and 0 < want[2, 3, 40] < 252
    assert np.array_equal(masks.feather(mask, width, device=hip_device), want)


def test_uniform_masks_and_no_feather(hip_device):
    assert np.all(masks.feather(np.full((3, 5, 33), 9, np.uint8), (2, 2, 9), device=hip_device) == masks.FULL_WEIGHT)
    assert np.all(masks.feather(np.zeros((5, 33), np.uint8), 7, device=hip_device) == 0)
    mask = np.array(fc.blob_mask((6, 11, 37)))
    assert np.array_equal(masks.feather(mask, 0, device=hip_device), mask * np.uint8(252))
    assert np.array_equal(masks.feather(mask * np.uint8(200), (1, 1, 1), device=hip_device), mask * np.uint8(252))      # nonzero means "use"


def test_strided_device_window(hip_device):
    """A window of a larger device array: rows start 3 voxels off the 16-byte grid and keep the parent's pitch."""
    parent = np.array(fc.blob_mask((7, 21, 70), seed=9))
    window = DeviceArray.from_host(parent, hip_device)[1:, 2:, 3:]
    assert not window.is_contiguous()
    want = oracle(parent[1:, 2:, 3:], (2, 5, 12))
    got = _mask_ops.feather(window, (2, 5, 12), hip_device)
    assert np.array_equal(got, want)
    with pytest.raises(TypeError, match="contiguous"):
        masks.feather(window, (2, 5, 12), device=hip_device)


@pytest.mark.parametrize("planes", [1, 2, 5])
def test_slabs_do_not_change_a_byte(planes, hip_device):
    shape, width = (13, 20, 37), (3, 8, 8)
    mask = np.array(fc.blob_mask(shape))
    whole = masks.feather(mask, width, device=hip_device)
    assert np.array_equal(whole, oracle(mask, width))
    _lib.set_option("feather_slab_planes", planes, hip_device)
    try:
        slabbed = masks.feather(mask, width, device=hip_device)
    finally:
        _lib.set_option("feather_slab_planes", 0, hip_device)
    assert np.array_equal(slabbed, whole)


def test_sims_keep_their_coordinates(hip_device):
    mask = np.array(fc.blob_mask((33, 50)))
    sim = si.to_spatial_image(mask, dims=["y", "x"], scale={"y": 2.0, "x": 0.5}, translation={"y": -3.0, "x": 10.0})
    si.set_sim_affine(sim, np.eye(3), "stage")
    got = masks.feather(sim, {"y": 4, "x": 17}, device=hip_device)
    assert list(got.dims) == ["y", "x"] and "stage" in got.attrs["transforms"]
    for d in ("y", "x"):
        assert np.array_equal(np.asarray(got.coords[d]), np.asarray(sim.coords[d]))
    assert np.array_equal(np.asarray(got.data), oracle(mask, (4, 17)))
