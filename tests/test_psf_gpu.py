"""GPU: mv_deconv.extract_psf / extract_psfs (mvs_psf_extract, csrc/mvs_psf.hip) against the numpy / scipy restatement
(tests/psf_oracle.py): fixture A in three dtypes and from device memory, a rotated anisotropic window, the rejection statuses,
the window sizes at the kernel's edges, argument errors of the raw entry, determinism across runs and batch sizes, and the
detect -> attach -> extract -> deconvolve sequence end to end.

Bounds (all from the sampler's float32 tap weights: a relative 2^-24 per product, a few 1e-7 per sample; a centroid over
|o| <= 6 turns that into a few 1e-6 px):  PSF and ncc  |got - want| <= 1e-4 max(|want|, 1e-3 range(want));  centres 1e-4 px."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import psf_oracle as po

pytestmark = pytest.mark.gpu

ROT_X = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])      # 90 degrees about x (z, y, x order)
M_ROT = np.array([[0.0, 0.5, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    if nan.all():
        return
    rng = want[~nan].max() - want[~nan].min()
    bound = 1e-4 * np.maximum(np.abs(want[~nan]), 1e-3 * rng)
    err = np.abs(got[~nan] - want[~nan])
    print(f"{what}: max error / bound = {(err / bound).max():.3e} (max error {err.max():.3e})")
    assert np.all(err <= bound), what


def _centers_close(got, want, what):
    err = np.abs(np.asarray(got) - np.asarray(want)).max()
    print(f"{what}: centres differ by at most {err:.3e} px")
    assert err <= 1e-4


def _sim(data, spacing=None, origin=None):
    from multiview_stitcher_amd import spatial_image_utils as si

    dims = ["z", "y", "x"][-len(data.shape):]
    spacing = [1.0] * len(dims) if spacing is None else spacing
    origin = [0.0] * len(dims) if origin is None else origin
    return si.to_spatial_image(data, dims=dims, scale=dict(zip(dims, spacing)), translation=dict(zip(dims, origin)))


def _compare(got, want, spacing, what):
    """(psf, info) of extract_psf(return_info=True) against the restatement's."""
    assert got[1]["status"] == want[1]["status"], what
    assert got[1]["n_used"] == want[1]["n_used"]
    assert got[0].dtype == np.float32 and abs(float(got[0].sum(dtype=np.float64)) - 1.0) < 1e-6
    _close(got[0], want[0], what + " PSF")
    _close(got[1]["ncc"], want[1]["ncc"], what + " ncc")
    _close(got[1]["background"], want[1]["background"], what + " background")
    _centers_close(got[1]["centers"] / np.asarray(spacing), want[1]["centers"] / np.asarray(spacing), what)


# ---- fixture A ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_a(dtype_name, min_correlation):
    """View, positions and the restatement's result, computed once and left unchanged."""
    view, truth, given = po.fixture_a(np.dtype(dtype_name))
    want = po.extract_psf(view, (1, 1, 1), (0, 0, 0), given, (13, 9, 11), min_correlation=min_correlation)
    for a in (view, truth, given, want[0]):
        a.setflags(write=False)
    return view, given, want


@pytest.mark.parametrize("min_correlation", [None, po.FIXTURE_A_MIN_CORRELATION], ids=["all", "ncc0.97"])
@pytest.mark.parametrize("dtype,mem", [("float32", "host"), ("uint16", "host"), ("uint8", "host"), ("uint16", "device")])
def test_fixture_a(hip_device, dtype, mem, min_correlation):
    from multiview_stitcher_amd import mv_deconv
    from multiview_stitcher_amd.device import DeviceArray

    view, given, want = _fixture_a(dtype, min_correlation)
    data = DeviceArray.from_host(view, hip_device) if mem == "device" else view
    got = mv_deconv.extract_psf(_sim(data), given, (13, 9, 11), min_correlation=min_correlation, device=hip_device, return_info=True)
    not_used = [i for i, s in enumerate(got[1]["status"]) if s != "used"]
    assert not_used == ([] if min_correlation is None else [po.FIXTURE_A_DOUBLET])
    if min_correlation is not None:
        assert got[1]["status"][po.FIXTURE_A_DOUBLET] == "low_correlation"
    _compare(got, want, (1, 1, 1), f"fixture A {dtype} {mem}")
    assert mv_deconv.extract_psf(_sim(data), given, (13, 9, 11), min_correlation=min_correlation, device=hip_device).tobytes() == got[0].tobytes()


# ---- a window that is rotated and anisotropic in the view ---------------------------------------------------------------------------
def test_rotated_anisotropic_window(hip_device):
    """View spacing (2, 1, 1), rotated 90 degrees about x against the output grid of spacing 1: M = [[0, .5, 0], [-1, 0, 0], [0, 0, 1]].
    A transposed or inverted M samples other voxels."""
    from multiview_stitcher_amd import mv_deconv

    rng = np.random.default_rng(12)
    spacing, origin = (2.0, 1.0, 1.0), (3.0, -2.0, 5.0)
    lattice = np.array([(6, 10, 10), (6, 10, 28), (6, 28, 10), (16, 28, 28), (16, 10, 28), (16, 28, 10)], dtype=np.float64)
    truth = lattice + rng.uniform(-0.4, 0.4, lattice.shape)
    view = po.gaussian_beads((24, 40, 40), truth, rng.uniform(800.0, 2500.0, 6), (0.7, 1.3, 1.1), 60.0).astype(np.float32)
    points = np.asarray(origin) + np.rint(truth * 2) / 2 * np.asarray(spacing)
    kw = dict(affine=ROT_X, output_spacing={"z": 1.0, "y": 1.0, "x": 1.0}, refine_iterations=2)
    want = po.extract_psf(view, spacing, origin, points, (7, 7, 7), affine=ROT_X, output_spacing=(1.0, 1.0, 1.0), refine_iterations=2)
    assert want[1]["status"] == ["used"] * 6
    np.testing.assert_allclose(po.window_matrix(spacing, ROT_X, (1.0, 1.0, 1.0)), M_ROT, atol=1e-15)
    got = mv_deconv.extract_psf(_sim(view, spacing, origin), points, (7, 7, 7), device=hip_device, return_info=True, **kw)
    _compare(got, want, spacing, "rotated window")
    wrong = po.extract_psf(view, spacing, origin, points, (7, 7, 7), affine=ROT_X.T, output_spacing=(1.0, 1.0, 1.0), refine_iterations=2)[0]
    assert np.abs(wrong - want[0]).max() > 1e-2 * want[0].max()      # (the comparison above would see a transposed M)


# ---- rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections(hip_device):
    """A window that leaves the view at the given centre, one that leaves it only after the refinement, and a bead that stays."""
    from multiview_stitcher_amd import mv_deconv

    truth = np.array([[5.2, 10.0, 12.0], [5.6, 10.0, 40.0], [20.0, 30.0, 27.0], [21.3, 12.4, 41.8]])
    view = po.gaussian_beads((40, 48, 56), truth, [1500.0, 1800.0, 1200.0, 2000.0], (2.0, 1.2, 1.5), 100.0).astype(np.float32)
    given = truth.copy()
    given[1:] = np.rint(truth[1:])      # bead 1: z = 6, the window [0, 12] fits; refined to 5.6 it does not
    want = po.extract_psf(view, (1, 1, 1), (0, 0, 0), given, (13, 9, 11))
    assert want[1]["status"] == ["outside", "outside", "used", "used"]
    got = mv_deconv.extract_psf(_sim(view), given, (13, 9, 11), device=hip_device, return_info=True)
    _compare(got, want, (1, 1, 1), "rejections")
    assert got[1]["centers"][0].tolist() == given[0].tolist() and abs(got[1]["centers"][1][0] - 5.6) < 0.05
    unrefined = mv_deconv.extract_psf(_sim(view), given, (13, 9, 11), refine_iterations=0, device=hip_device, return_info=True)[1]
    assert unrefined["status"] == ["outside", "used", "used", "used"]


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_a_constant_view_has_no_usable_bead(hip_device, dtype):
    from multiview_stitcher_amd import _psf_ops, mv_deconv

    view = np.full((20, 24, 28), 100, dtype=dtype)
    pts = np.array([[8.0, 9.0, 10.0], [10.0, 14.0, 20.0]])      # (whole voxels: a sample is a voxel, exactly)
    psf, centers, status, stats = _psf_ops.psf_extract(view, pts, np.eye(3), (2, 3, 4), 1, hip_device)
    assert status.tolist() == [_psf_ops.STATUS_EMPTY] * 2 and not psf.any()
    assert stats[:, 0].tolist() == [100.0, 100.0] and stats[:, 1].tolist() == [0.0, 0.0] and np.isnan(stats[:, 2]).all()
    np.testing.assert_array_equal(centers, pts)
    with pytest.raises(ValueError, match="no usable bead"):
        mv_deconv.extract_psf(_sim(view), pts, (5, 7, 9), device=hip_device)


# ---- window sizes at the kernel's edges ---------------------------------------------------------------------------------------------
def test_smallest_window(hip_device):
    """Radius (1, 1, 1): 27 offsets, less than one wave."""
    from multiview_stitcher_amd import mv_deconv

    view, given, _ = _fixture_a("float32", None)
    want = po.extract_psf(view, (1, 1, 1), (0, 0, 0), given, (3, 3, 3))
    got = mv_deconv.extract_psf(_sim(view), given, (3, 3, 3), device=hip_device, return_info=True)
    _compare(got, want, (1, 1, 1), "radius (1, 1, 1)")


def test_two_dimensions(hip_device):
    from multiview_stitcher_amd import mv_deconv

    rng = np.random.default_rng(21)
    lattice = np.array([(y, x) for y in (8, 22, 34) for x in (12, 34, 56)], dtype=np.float64)
    truth = lattice + rng.uniform(-0.5, 0.5, lattice.shape)
    view = np.rint(po.gaussian_beads((44, 70), truth, rng.uniform(500.0, 3000.0, 9), (1.4, 2.6), 90.0)).astype(np.uint16)
    spacing, origin = (0.5, 0.25), (10.0, -4.0)
    points = np.asarray(origin) + np.rint(truth) * np.asarray(spacing)
    want = po.extract_psf(view, spacing, origin, points, (9, 15))
    assert want[1]["status"] == ["used"] * 9
    got = mv_deconv.extract_psf(_sim(view, spacing, origin), points, {"y": 9, "x": 15}, device=hip_device, return_info=True)
    assert got[0].shape == (9, 15)
    _compare(got, want, spacing, "2D radius (4, 7)")


def test_longest_window_and_a_single_bead(hip_device):
    """Radius (1, 1, 31) -- 63 samples along x, the limit -- on an 8 x 8 x 200 view, with n_beads = 1."""
    from multiview_stitcher_amd import mv_deconv

    truth = np.array([[3.7, 4.2, 100.4]])
    view = po.gaussian_beads((8, 8, 200), truth, [2000.0], (0.8, 0.8, 9.0), 50.0).astype(np.float32)
    given = np.rint(truth)
    want = po.extract_psf(view, (1, 1, 1), (0, 0, 0), given, (3, 3, 63))
    assert want[1]["status"] == ["used"]
    got = mv_deconv.extract_psf(_sim(view), given, (3, 3, 63), device=hip_device, return_info=True)
    assert got[0].shape == (3, 3, 63)
    _compare(got, want, (1, 1, 1), "radius (1, 1, 31)")
    assert abs(got[1]["ncc"][0] - 1.0) < 1e-6      # one bead is its own average


def test_the_raw_entry_refuses_bad_arguments(hip_device):
    """Returned codes, never a crash: radius 0 on a used axis, radius 32, a NULL pointer, ndim 4, a 2D view with planes, no bead."""
    from multiview_stitcher_amd import _lib

    lib = _lib.init(hip_device)
    data = np.full((6, 8, 10), 7, np.uint16)
    view = _lib.mvs_view_t()
    view.data, view.dtype, view.mem = data.ctypes.data, _lib.MVS_U16, _lib.MVS_MEM_HOST
    view.shape[:] = data.shape
    view.stride[:] = [80, 10, 1]
    centers = np.array([[3.0, 4.0, 5.0]])
    eye = np.eye(3).reshape(9)
    out_c, status, stats, psf = np.zeros((1, 3)), np.zeros(1, np.int32), np.zeros((1, 3), np.float32), np.zeros(65 ** 3, np.float32)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def call(ndim=3, radius=(1, 1, 1), n=1, centers_ptr=centers.ctypes.data_as(dp), psf_ptr=psf.ctypes.data_as(fp), refine=1):
        return lib.mvs_psf_extract(hip_device, C.byref(view), ndim, centers_ptr, n, eye.ctypes.data_as(dp), (C.c_int32 * 3)(*radius), refine,
                                   out_c.ctypes.data_as(dp), status.ctypes.data_as(ip), stats.ctypes.data_as(fp), psf_ptr)

    assert call() == 0 and status[0] == 2      # (a constant view: the bead is empty, the call itself is fine)
    assert call(radius=(0, 1, 1)) == -1 and b"radius" in lib.mvs_last_error(hip_device)
    assert call(radius=(1, 1, 0)) == -1
    assert call(radius=(1, 32, 1)) == -1
    assert call(radius=(-1, 1, 1)) == -1
    assert call(centers_ptr=None) == -1 and call(psf_ptr=None) == -1
    assert call(ndim=4) == -1 and call(ndim=1) == -1
    assert call(ndim=2) == -1                  # shape[0] == 6
    assert call(n=0) == -1 and call(n=-3) == -1
    assert call(refine=-1) == -1
    with pytest.raises(_lib.MvsError):
        _lib.set_option("psf_batch", -1, hip_device)
    assert call() == 0


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_runs_and_batch_sizes_give_identical_bytes(hip_device):
    from multiview_stitcher_amd import _lib, _psf_ops

    view, given, _ = _fixture_a("uint16", None)

    def run():
        return b"".join(np.ascontiguousarray(a).tobytes() for a in _psf_ops.psf_extract(view, given, np.eye(3), po.FIXTURE_A_RADIUS, 1, hip_device))

    first = run()
    assert run() == first
    try:
        for batch in (1, 5):
            _lib.set_option("psf_batch", batch, hip_device)
            assert run() == first, f"psf_batch = {batch}"
    finally:
        _lib.set_option("psf_batch", 0, hip_device)
    assert run() == first


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_detect_extract_deconvolve(hip_device):
    """Two 32 x 40 x 40 views of one bead field, the second rotated 90 degrees about x: detect_beads -> set_point_set ->
    extract_psfs -> fuse(multi_view_deconvolution, psfs).  The PSFs are the restatement's for the detected points; the fuse runs."""
    from multiview_stitcher_amd import detection, fusion, msi_utils, mv_deconv
    from multiview_stitcher_amd import spatial_image_utils as si

    rng = np.random.default_rng(8)
    world = np.array([(z, y, x) for z in (10, 22) for y in (14, 26) for x in (10, 30)], dtype=np.float64) + rng.uniform(-0.4, 0.4, (8, 3))
    amps = rng.uniform(900.0, 2500.0, 8)
    second = ROT_X.copy()
    second[:3, 3] = (39.0, 4.0, 0.0)      # world = R p + t: the view's y axis runs down the world's z
    affines = [np.eye(4), second]
    msims, views = [], []
    for a in affines:
        local = (np.linalg.inv(a) @ np.c_[world, np.ones(8)].T).T[:, :3]
        view = np.rint(po.gaussian_beads((32, 40, 40), local, amps, (1.3, 1.3, 1.3), 120.0)).astype(np.uint16)
        sim = si.get_sim_from_array(view, dims=["z", "y", "x"], scale=dict(zip("zyx", (1.0, 1.0, 1.0))), translation=dict(zip("zyx", (0.0, 0.0, 0.0))),
                                    affine=a, transform_key="registered")
        msims.append(msi_utils.get_msim_from_sim(sim))
        views.append(view)
    for msim in msims:
        points = detection.detect_beads(msim, detection_func_kwargs={"target_size_physical": 4.0}, device=hip_device)
        assert len(points) == 8
        msi_utils.set_point_set(msim, points)
    psfs = mv_deconv.extract_psfs(msims, "registered", (7, 7, 7), device=hip_device)
    assert len(psfs) == 2
    for v in range(2):
        want = po.extract_psf(views[v], (1, 1, 1), (0, 0, 0), msi_utils.get_point_set(msims[v]), (7, 7, 7), affine=affines[v], output_spacing=(1, 1, 1))
        assert want[1]["status"] == ["used"] * 8
        assert psfs[v].shape == (7, 7, 7) and psfs[v].dtype == np.float32
        _close(psfs[v], want[0], f"end to end, view {v}")
    sims = [msi_utils.get_sim_from_msim(m) for m in msims]
    fused = fusion.fuse(sims, transform_key="registered", fusion_func=fusion.multi_view_deconvolution,
                        fusion_func_kwargs={"psfs": psfs, "n_iterations": 2}, device=hip_device)
    want_shape = fusion.process_output_stack_properties(sims, transform_key="registered")["shape"]
    out = np.asarray(fused.data)
    assert out.shape[-3:] == tuple(want_shape[d] for d in "zyx") and out.dtype == np.uint16
    assert np.isfinite(out.astype(np.float64)).all() and out.max() > 120
