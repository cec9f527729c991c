"""Arrays whose upload is still in flight, handed straight to the wrappers (``_operands.py``: every wrapper makes its stream wait)."""
import numpy as np
import pytest
from scipy import ndimage

from multiview_stitcher_amd import _reg_ops, device, transformation
from multiview_stitcher_amd import spatial_image_utils as si

pytestmark = pytest.mark.gpu

MATRIX, OFFSET, OUT_SHAPE = np.diag([1.0, 1.1, 0.9]), np.array([0.5, -1.25, 2.0]), (7, 20, 33)


def test_arrays_from_to_device_async_go_into_the_wrappers_without_a_host_wait(hip_device):
    """A pinned (8, 24, 40) float32 pair is uploaded with ``to_device_async`` and passed on at once, with no ``sync_ready``, to
    ``phase_cross_correlation``, ``rescale_intensity(out_on_device=True)`` and ``resample_array`` -- a fresh upload for each, so that
    each call meets one that may still be in flight.  The results are those of the host inputs: the same shift, bit-identical arrays.

    A guard, not a reproducer: without the wait in the wrapper the kernel races a 30 KB copy, and the copy may well win, so the code
    before the wrappers waited can pass this test too."""
    scene = ndimage.gaussian_filter(np.random.default_rng(7).random((12, 30, 46)), 1.0).astype(np.float32)
    hosts = [np.ascontiguousarray(scene[2:10, 3:27, 3:43]), np.ascontiguousarray(scene[3:11, 1:25, 5:45])]
    assert hosts[0].shape == (8, 24, 40)

    def uploading():
        sims = []
        for h in hosts:
            staged = device.pinned_empty(h.shape, h.dtype)
            staged[:] = h
            sims.append(si.to_spatial_image(h, dims=["z", "y", "x"], scale=dict(zip("zyx", (1.0, 1.0, 1.0))),
                                            translation=dict(zip("zyx", (0.0, 0.0, 0.0)))).copy(data=staged))
        arrays = [s.data for s in device.to_device_async(sims, hip_device)]
        assert all(a.ready_ticket for a in arrays)
        return arrays

    want_shift = _reg_ops.phase_cross_correlation(*hosts, upsample_factor=10, device=hip_device)
    want_rescaled = _reg_ops.rescale_intensity(hosts[0], hip_device)
    want_resampled = transformation.resample_array(hosts[1], MATRIX, OFFSET, OUT_SHAPE, device=hip_device)
    assert np.abs(want_shift).max() > 0 and isinstance(want_resampled, np.ndarray) and np.count_nonzero(want_resampled) > 0

    a, b = uploading()
    got_shift = _reg_ops.phase_cross_correlation(a, b, upsample_factor=10, device=hip_device)
    assert np.array_equal(got_shift, want_shift)

    a, _ = uploading()
    got, mn, mx, nv = _reg_ops.rescale_intensity(a, hip_device, out_on_device=True)
    assert (mn, mx, nv) == want_rescaled[1:] and got.get().tobytes() == want_rescaled[0].tobytes()

    _, b = uploading()
    got = transformation.resample_array(b, MATRIX, OFFSET, OUT_SHAPE, device=hip_device)
    assert device.is_device_array(got) and got.get().tobytes() == want_resampled.tobytes()
