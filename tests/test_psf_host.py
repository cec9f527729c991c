"""CPU tests of the PSF extraction from beads: the numpy / scipy restatement itself (tests/psf_oracle.py) on cases whose answer is
known, the host geometry of mv_deconv.extract_psf (window matrix, separation rule, argument errors raised before any device work),
and that such PSFs are what mv_deconv._kernels takes."""
import numpy as np
import pytest

from tests import psf_oracle as po


def _sim(data, spacing=None, origin=None):
    from multiview_stitcher_amd import spatial_image_utils as si

    dims = ["z", "y", "x"][-data.ndim:]
    spacing = [1.0] * data.ndim if spacing is None else spacing
    origin = [0.0] * data.ndim if origin is None else origin
    return si.to_spatial_image(data, dims=dims, scale=dict(zip(dims, spacing)), translation=dict(zip(dims, origin)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_oracle_at_integer_positions_is_the_mean_of_the_normalised_crops():
    """M = I, integer centres, no refinement: every sample is a voxel, so the PSF is the plain mean of the background-subtracted
    crops, each scaled to unit sum -- exactly."""
    rng = np.random.default_rng(0)
    view = (rng.random((20, 24, 26)) * 900.0 + 50.0).astype(np.float32)
    centers = np.array([[5, 6, 7], [13, 17, 19], [9, 11, 12], [15, 4, 21]])
    radius = (2, 3, 4)
    _, shell = po.offsets(radius)
    shell = shell.reshape(5, 7, 9)
    acc = np.zeros((5, 7, 9))
    for c in centers:
        crop = view[tuple(slice(ci - r, ci + r + 1) for ci, r in zip(c, radius))].astype(np.float64)
        e = np.maximum(crop - crop[shell].mean(), 0.0)
        acc = acc + e / e.sum()
    got = po.extract(view, centers, np.eye(3), radius, refine_iterations=0)
    assert got["status"] == ["used"] * 4
    np.testing.assert_array_equal(got["psf"], acc / 4)
    np.testing.assert_array_equal(got["centers"], centers.astype(np.float64))


@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.uint8], ids=lambda d: np.dtype(d).name)
def test_oracle_on_fixture_a(dtype):
    """All 18 beads used; one refinement brings every clean bead closer to its true position than the rounded input (to within
    0.004 px for float32 / uint16 data); the doublet correlates worse with the average than every clean bead, on either side of
    the threshold the GPU tests use."""
    view, truth, given = po.fixture_a(dtype)
    res = po.extract(view, given, np.eye(3), po.FIXTURE_A_RADIUS, refine_iterations=1)
    assert res["status"] == ["used"] * 18
    clean = [b for b in range(18) if b != po.FIXTURE_A_DOUBLET]
    before = np.abs(given - truth).max(axis=1)
    after = np.abs(res["centers"] - truth).max(axis=1)
    assert np.all(after[clean] < before[clean])
    if dtype != np.uint8:
        assert after[clean].max() < 0.004
    ncc = res["ncc"]
    assert ncc[po.FIXTURE_A_DOUBLET] < po.FIXTURE_A_MIN_CORRELATION < ncc[clean].min()
    assert ncc[clean].min() >= 0.9988 and abs(ncc[po.FIXTURE_A_DOUBLET] - 0.944) < 1e-3
    psf, info = po.extract_psf(view, (1, 1, 1), (0, 0, 0), given, (13, 9, 11), min_correlation=po.FIXTURE_A_MIN_CORRELATION)
    assert [i for i, s in enumerate(info["status"]) if s != "used"] == [po.FIXTURE_A_DOUBLET]
    assert info["status"][po.FIXTURE_A_DOUBLET] == "low_correlation" and info["n_used"] == 17
    assert psf.dtype == np.float32 and psf.shape == (13, 9, 11) and abs(float(psf.sum(dtype=np.float64)) - 1.0) < 1e-6
    assert np.unravel_index(psf.argmax(), psf.shape) == (6, 4, 5)


# ---- host geometry ----------------------------------------------------------------------------------------------------------------
ROT_X = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])      # 90 degrees about x (z, y, x order)
M_ROT = np.array([[0.0, 0.5, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def test_window_matrix_of_a_rotated_anisotropic_view():
    from multiview_stitcher_amd import _psf_ops

    np.testing.assert_allclose(_psf_ops.window_matrix((2.0, 1.0, 1.0), ROT_X[:3, :3], (1.0, 1.0, 1.0)), M_ROT, atol=1e-15)
    np.testing.assert_allclose(po.window_matrix((2.0, 1.0, 1.0), ROT_X, (1.0, 1.0, 1.0)), M_ROT, atol=1e-15)
    shifted = ROT_X.copy()
    shifted[:3, 3] = (7.0, -3.0, 11.0)      # the translation does not enter
    np.testing.assert_array_equal(po.window_matrix((2.0, 1.0, 1.0), shifted, (1.0, 1.0, 1.0)), po.window_matrix((2.0, 1.0, 1.0), ROT_X, (1.0, 1.0, 1.0)))
    with pytest.raises(ValueError, match="singular"):
        _psf_ops.window_matrix((1.0, 1.0, 1.0), np.diag([1.0, 0.0, 1.0]), (1.0, 1.0, 1.0))


def test_separation_rule():
    """Two beads 10 px apart along x with r_x = 5 sit in each other's windows (10 < 11): both go.  At 11 px both stay.  The k-d tree
    form agrees with the chunked restatement on random points under a rotated, anisotropic window matrix."""
    from multiview_stitcher_amd import _psf_ops

    radius = (2, 3, 5)
    far = [30.0, 40.0, 90.0]
    for gap, want in ((10.0, [True, True, False]), (11.0, [False, False, False])):
        centers = np.array([[5.0, 6.0, 20.0], [5.0, 6.0, 20.0 + gap], far])
        assert _psf_ops.too_close(centers, np.eye(3), radius).tolist() == want
        assert po.too_close(centers, np.eye(3), radius).tolist() == want
    pts = np.random.default_rng(5).uniform(0.0, 110.0, (700, 3))
    got = _psf_ops.too_close(pts, M_ROT, (3, 2, 4))
    assert 100 < got.sum() < 600      # (a mix of both outcomes)
    np.testing.assert_array_equal(got, po.too_close(pts, M_ROT, (3, 2, 4)))
    assert _psf_ops.too_close(pts[:1], M_ROT, (3, 2, 4)).tolist() == [False]


def test_argument_errors_come_before_any_device_work(monkeypatch):
    from multiview_stitcher_amd import _psf_ops, mv_deconv

    def no_device(*a, **k):
        raise AssertionError("the device entry was called")

    monkeypatch.setattr(_psf_ops, "psf_extract", no_device)
    sim = _sim(np.zeros((12, 14, 16), np.uint16))
    pts = np.array([[6.0, 7.0, 8.0]])
    with pytest.raises(ValueError, match="singular"):
        mv_deconv.extract_psf(sim, pts, (5, 5, 5), affine=np.diag([1.0, 1.0, 0.0, 1.0]))
    for bad in ((4, 5, 5), (5, 5, 65), (1, 5, 5), {"z": 5, "y": 6, "x": 5}, (5, 5)):
        with pytest.raises(ValueError, match="psf_shape"):
            mv_deconv.extract_psf(sim, pts, bad)
    for bad in (np.zeros((3, 2)), np.zeros(3), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match="points"):
            mv_deconv.extract_psf(sim, bad, (5, 5, 5))
    with pytest.raises(ValueError, match="no bead"):      # two beads, each in the other's window
        mv_deconv.extract_psf(sim, np.array([[6.0, 7.0, 8.0], [6.0, 7.0, 9.0]]), (5, 5, 5))
    with pytest.raises(AssertionError, match="device entry"):      # (valid arguments do reach the device entry)
        mv_deconv.extract_psf(sim, pts, {"z": 5, "y": 5, "x": 5})


def test_separation_and_max_beads_decide_what_reaches_the_device(monkeypatch):
    """extract_psf hands the device entry the pixel centres of the beads that pass the separation rule, the first max_beads of
    them, with the window matrix of the view; the statuses of the others say why they were left out."""
    from multiview_stitcher_amd import _psf_ops, mv_deconv

    seen = {}

    def fake(data, centers, matrix, radius, refine_iterations, device):
        seen.update(centers=np.array(centers), matrix=np.array(matrix), radius=list(radius), refine=refine_iterations)
        n = len(centers)
        psf = np.zeros(tuple(2 * r + 1 for r in radius), np.float32)
        psf[tuple(radius)] = 2.0
        stats = np.tile(np.array([[10.0, 5.0, 0.99]], np.float32), (n, 1))
        return psf, np.array(centers) + 0.25, np.zeros(n, np.int32), stats

    monkeypatch.setattr(_psf_ops, "psf_extract", fake)
    sim = _sim(np.zeros((30, 40, 40), np.uint16), spacing=(2.0, 1.0, 1.0), origin=(3.0, -2.0, 5.0))
    centers = np.array([[8.0, 10.0, 10.0], [8.0, 10.0, 12.0], [20.0, 30.0, 30.0], [20.0, 12.0, 30.0], [9.0, 30.0, 9.0]])
    points = np.array([3.0, -2.0, 5.0]) + centers * np.array([2.0, 1.0, 1.0])
    psf, info = mv_deconv.extract_psf(sim, points, (7, 7, 7), affine=ROT_X, output_spacing={"z": 1.0, "y": 1.0, "x": 1.0}, max_beads=2,
                                      refine_iterations=3, return_info=True)
    assert info["status"] == ["too_close", "too_close", "used", "used", "skipped"] and info["n_used"] == 2
    np.testing.assert_allclose(seen["centers"], centers[2:4], atol=1e-12)
    np.testing.assert_allclose(seen["matrix"], M_ROT, atol=1e-15)
    assert seen["radius"] == [3, 3, 3] and seen["refine"] == 3
    np.testing.assert_allclose(info["centers"][2:4], points[2:4] + 0.25 * np.array([2.0, 1.0, 1.0]), atol=1e-12)
    np.testing.assert_array_equal(info["centers"][[0, 1, 4]], points[[0, 1, 4]])
    assert np.isnan(info["ncc"][[0, 1, 4]]).all() and np.allclose(info["ncc"][2:4], 0.99)
    assert psf.dtype == np.float32 and psf.sum() == 1.0      # through _norm


def test_measured_psfs_are_what_the_deconvolution_takes():
    """PSFs of the form extract_psfs returns (here: the restatement's, one per dtype of fixture A) pass mv_deconv._kernels: the
    views' dimension, odd, at most 63 per axis, float32, unit sum."""
    from multiview_stitcher_amd import mv_deconv

    psfs = []
    for dtype in (np.float32, np.uint16):
        view, _, given = po.fixture_a(dtype)
        psfs.append(po.extract_psf(view, (1, 1, 1), (0, 0, 0), given, (13, 9, 11))[0])
    k1, k2, _, _ = mv_deconv._kernels(2, 3, psfs, mv_deconv.PSFType.EFFICIENT_BAYESIAN, None, 0.8, 0.5)
    assert k1.shape == k2.shape == (2, 13, 9, 11) and k1.dtype == np.float32
    for v in range(2):
        assert psfs[v].ndim == 3 and all(n % 2 == 1 and n <= mv_deconv.KERNEL_LIMIT for n in psfs[v].shape)
        assert abs(float(k1[v].sum(dtype=np.float64)) - 1.0) < 1e-6
        np.testing.assert_allclose(k1[v], psfs[v], rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        mv_deconv._kernels(2, 2, psfs, mv_deconv.PSFType.EFFICIENT_BAYESIAN, None, 0.8, 0.5)
