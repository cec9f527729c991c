"""GPU: every lane and every wave of a workgroup reaches the result of the kernels' shared fold (csrc/mvs_fold_dev.h).  One value
that differs from all others is put at a position owned by the first, the last and the boundary lanes of every wave of the first
workgroups in turn; a lane or a wave that the fold drops shows as a wrong minimum, maximum, count or peak index.  No tolerances:
the expected values come from numpy on the same array."""
import numpy as np
import pytest

from oracle import reg_oracle as ro

pytestmark = pytest.mark.gpu

N = 700
RANGE_POSITIONS = [0, 1, 31, 32, 63, 64, 127, 128, 191, 192, 255, 256, 511, 699]
PEAK_SHAPE = (8, 64)
PEAK_POSITIONS = [0, 1, 31, 32, 63, 64, 255, 256, 511]


def _range_functions():
    from multiview_stitcher_amd import _reg_ops

    return {"finite_range": lambda a: _reg_ops.finite_range(a),
            "rescale_intensity": lambda a: _reg_ops.rescale_intensity(a)[1:]}


def _residencies():
    from multiview_stitcher_amd.device import DeviceArray

    return {"host": lambda a: a, "device": lambda a: DeviceArray.from_host(a)}


@pytest.mark.parametrize("p", RANGE_POSITIONS)
def test_range_fold_sees_every_position(hip_device, p):
    for fname, f in _range_functions().items():
        for rname, put in _residencies().items():
            where = (fname, rname, p)
            a = np.ones(N, np.float32)
            a[p] = 2.0
            mn, mx, nv = f(put(a))
            assert (mn, mx, nv) == (float(a.min()), float(a.max()), N) == (1.0, 2.0, 700), where
            a[p] = 0.5
            mn, mx, nv = f(put(a))
            assert (mn, mx, nv) == (float(a.min()), float(a.max()), N) and mn == 0.5, where
            a = np.full(N, np.nan, np.float32)
            a[p] = 1.0
            mn, mx, nv = f(put(a))
            assert nv == int(np.isfinite(a).sum()) == 1 and mn == mx == float(np.nanmin(a)) == float(a[p]), where


@pytest.mark.parametrize("p", PEAK_POSITIONS)
def test_peak_fold_sees_every_position(hip_device, p):
    """A delta rolled to flat index p against the delta at the origin: their correlation is a delta at p."""
    from multiview_stitcher_amd import _reg_ops

    delta = np.zeros(PEAK_SHAPE, np.float32)
    delta[0, 0] = 1.0
    at = np.unravel_index(p, PEAK_SHAPE)
    rolled = np.roll(delta, at, axis=(0, 1))
    _, want = ro.phase_cross_correlation(rolled, delta, upsample_factor=1, normalization=None, return_debug=True)
    _, got = _reg_ops.phase_cross_correlation(rolled, delta, upsample_factor=1, normalization=None, return_debug=True)
    np.testing.assert_array_equal(got["peak_index"], want["peak_index"])
    np.testing.assert_array_equal(got["peak_index"], at)
