"""GPU: mvs_log_response against the scipy restatement (tests/detection_oracle.py) within a multiple of the restatement's own
float32 / float64 deviation, mvs_local_maxima exactly on volumes full of ties, log_detect / detect_beads end to end (labels
exactly, points to 1e-9, planted beads found), the neighbourhood-minimum rule, slabs, and two context lanes at once."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
from scipy import ndimage

from tests import detection_oracle as do

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
# (shape, target size in voxels)
CASES = [((40, 48), 5), ((20, 36, 44), (4, 5, 5)), ((33, 31, 29), (6, 3, 3)), ((3, 4, 130), 2), ((3, 4, 130), 6)]
CASE_IDS = ["2d-5", "3d-455", "3d-633", "thin-2", "thin-6"]
DTYPES = [np.uint8, np.uint16, np.float32]


def _target(shape, t):
    return float(t) if np.isscalar(t) else dict(zip("zyx"[-len(shape):], (float(v) for v in t)))


@functools.lru_cache(maxsize=None)
def _case(icase, dtype_name):
    """Image, planted positions and the restatement's results in both modes, computed once per case and left unchanged."""
    shape, t = CASES[icase]
    image, pos = do.make_beads(shape, t, seed=7 * len(shape) + int(np.sum(t)), dtype=np.dtype(dtype_name))
    spacing = (1.0,) * len(shape)
    want64 = do.log_detect(image, spacing, _target(shape, t), mode=np.float64, return_parts=True)
    want32 = do.log_detect(image, spacing, _target(shape, t), mode=np.float32, return_parts=True)
    for a in (image, pos) + want64[:3] + want32[:3]:
        a.setflags(write=False)
    return image, pos, spacing, _target(shape, t), want64, want32


def _put(a, mem, device):
    from multiview_stitcher_amd.device import DeviceArray

    return DeviceArray.from_host(a, device) if mem == "device" else a


# ---- 1. response ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("icase", range(len(CASES)), ids=CASE_IDS)
def test_response_matches_the_oracle(hip_device, icase, dtype, mem):
    """max |r - r64| / max |r64| <= 8x the same figure of the restatement's float32 mode (floor 4 eps32): the factor of
    test_affine_reg_gpu.py, for another pass structure and summation order.  The returned maximum is the volume's."""
    from multiview_stitcher_amd import _detect_ops

    image, _, spacing, target, want64, want32 = _case(icase, np.dtype(dtype).name)
    sigma, _, _ = do.parameters(spacing, target)
    got, got_max = _detect_ops.log_response(_put(image, mem, hip_device), sigma, float(np.mean(sigma)) ** 2, device=hip_device)
    r = got.get()
    r64 = want64[1]
    assert r.dtype == np.float32 and r.shape == r64.shape
    scale = np.abs(r64).max()
    err = np.abs(r.astype(np.float64) - r64).max() / scale
    dev = np.abs(want32[1].astype(np.float64) - r64).max() / scale
    print(f"response {CASE_IDS[icase]} {np.dtype(dtype).name} {mem}: error {err:.3e}, float32-mode deviation {dev:.3e}, ratio {err / max(dev, EPS32 / 2):.2f}")
    assert err <= max(8 * dev, 4 * EPS32)
    assert np.float32(got_max).tobytes() == r.max().tobytes()


def test_smoothing_is_the_order_zero_filter(hip_device):
    """The sample volume of max_neigh_sigma: mvs_log_response without the order-2 table is scipy's gaussian_filter."""
    from multiview_stitcher_amd import _detect_ops

    for icase, sigma in ((0, (1.3, 0.8)), (2, (0.7, 1.9, 1.1)), (4, (2.2, 0.6, 1.0))):
        image = _case(icase, "uint16")[0]
        got = _detect_ops.gaussian_smooth(image, sigma, device=hip_device).get()
        w64 = ndimage.gaussian_filter(image.astype(np.float64), sigma)
        w32 = ndimage.gaussian_filter(image.astype(np.float32), sigma)
        err, dev = np.abs(got - w64).max() / w64.max(), np.abs(w32 - w64).max() / w64.max()
        print(f"smoothing {CASE_IDS[icase]}: error {err:.3e}, float32-mode deviation {dev:.3e}")
        assert err <= max(8 * dev, 4 * EPS32)


def test_a_radius_above_the_limit_is_refused(hip_device):
    from multiview_stitcher_amd import _lib
    from multiview_stitcher_amd.device import DeviceArray

    lib = _lib.init(hip_device)
    image = np.zeros((4, 5, 6), np.float32)
    out = DeviceArray.empty(image.shape, np.float32, hip_device)
    r = _lib.MVS_LOG_MAX_RADIUS + 1
    taps = np.zeros(3 * (2 * r + 1))
    dp = taps.ctypes.data_as(C.POINTER(C.c_double))
    mx = C.c_float()
    call = lambda ndim, shape, radius, t0: lib.mvs_log_response(hip_device, image.ctypes.data, _lib.MVS_F32, _lib.MVS_MEM_HOST, ndim, _lib.i64x3(shape),   # noqa: E731
                                                                (C.c_int32 * 3)(*radius), t0, dp, 1.0, None, C.c_void_p(out.ptr), C.byref(mx))
    assert call(3, image.shape, (r, 1, 1), dp) == -4
    assert call(3, image.shape, (1, 1, -1), dp) == -1
    assert call(4, image.shape, (1, 1, 1), dp) == -1
    assert call(3, image.shape, (1, 1, 1), None) == -1
    assert call(2, image.shape, (1, 1, 1), dp) == -1           # 2D with an extent along z


# ---- 2. local maxima -------------------------------------------------------------------------------------------------------------
MAXIMA_CASES = [((5, 6, 7), (3, 5, 3)), ((17, 70), (3, 3)), ((3, 4, 130), (7, 3, 9)), ((1, 9, 300), (1, 3, 5))]


@functools.lru_cache(maxsize=None)
def _plateaus(shape):
    r = np.random.default_rng(sum(shape)).integers(0, 6, shape).astype(np.float32)
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("threshold", [0.0, 2.5])
@pytest.mark.parametrize("shape,window", MAXIMA_CASES, ids=lambda v: "x".join(map(str, v)))
def test_local_maxima_equal_scipy_on_plateaus(hip_device, shape, window, threshold):
    from multiview_stitcher_amd import _detect_ops
    from multiview_stitcher_amd.device import DeviceArray

    r = _plateaus(shape)
    want = np.argwhere(do.detections(r, window, threshold))
    dr = DeviceArray.from_host(r, hip_device)
    got = _detect_ops.local_maxima(dr, window, threshold, device=hip_device)
    assert len(want) > 0
    np.testing.assert_array_equal(got, want)
    for capacity in (None, max(len(want) // 2, 1)):      # run to run, and with a list that overflows on the way
        again = _detect_ops.local_maxima(dr, window, threshold, device=hip_device, capacity=capacity)
        assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("size", [2, 3, 4])
@pytest.mark.parametrize("sample_dtype", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape,window", MAXIMA_CASES, ids=lambda v: "x".join(map(str, v)))
def test_local_maxima_with_the_neighbourhood_minimum_rule(hip_device, shape, window, size, sample_dtype):
    from multiview_stitcher_amd import _detect_ops
    from multiview_stitcher_amd.device import DeviceArray

    r = _plateaus(shape)
    sample = np.random.default_rng(1 + sum(shape)).integers(0, 50, shape).astype(sample_dtype)
    plain = do.detections(r, window, 0.0)
    lowest = ndimage.minimum_filter(sample, size=size, mode="reflect")[plain]
    bound = float(np.median(lowest)) + 0.5
    want = np.argwhere(do.detections(r, window, 0.0, sample, bound, size))
    assert 0 < len(want) < plain.sum()
    got = _detect_ops.local_maxima(DeviceArray.from_host(r, hip_device), window, 0.0, DeviceArray.from_host(sample, hip_device),
                                   (size,) * len(shape), bound, device=hip_device)
    np.testing.assert_array_equal(got, want)


def _maxima_call(lib, device, dr, ndim, shape3, window, buf, capacity):
    count = C.c_int64(-1)
    rc = lib.mvs_local_maxima(device, C.c_void_p(dr.ptr), ndim, (C.c_int64 * 3)(*shape3), (C.c_int32 * 3)(*window), 0.0, None, 2, None, 0.0,
                              None if buf is None else buf.ctypes.data_as(C.POINTER(C.c_int32)), capacity, C.byref(count))
    return rc, count.value


def test_capacity_overflow_reports_the_exact_count(hip_device):
    from multiview_stitcher_amd import _detect_ops, _lib
    from multiview_stitcher_amd.device import DeviceArray

    lib = _lib.init(hip_device)
    ones = np.ones((5, 6, 7), np.float32)
    dr = DeviceArray.from_host(ones, hip_device)
    buf = np.full((17, 3), -7, np.int32)
    rc, count = _maxima_call(lib, hip_device, dr, 3, ones.shape, (3, 3, 3), buf, 16)
    assert rc == 0 and count == 210
    assert (buf[16] == -7).all() and (buf[:16] >= 0).all() and len({tuple(v) for v in buf[:16]}) == 16
    got = _detect_ops.local_maxima(dr, (3, 3, 3), 0.0, device=hip_device, capacity=16)
    np.testing.assert_array_equal(got, np.argwhere(ones > 0))


def test_local_maxima_refuses_bad_arguments(hip_device):
    from multiview_stitcher_amd import _lib
    from multiview_stitcher_amd.device import DeviceArray

    lib = _lib.init(hip_device)
    ones = np.ones((5, 6, 7), np.float32)
    dr = DeviceArray.from_host(ones, hip_device)
    buf = np.zeros((16, 3), np.int32)
    assert _maxima_call(lib, hip_device, dr, 4, ones.shape, (3, 3, 3), buf, 16)[0] < 0
    assert _maxima_call(lib, hip_device, dr, 3, ones.shape, (3, 4, 3), buf, 16)[0] < 0
    assert _maxima_call(lib, hip_device, dr, 3, ones.shape, (3, 3, 3), None, 16)[0] < 0
    assert _maxima_call(lib, hip_device, dr, 3, ones.shape, (3, 3, 3), None, 0) == (0, 210)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
def _msim(image, origin=None, spacing=None):
    from multiview_stitcher_amd import msi_utils
    from multiview_stitcher_amd import spatial_image_utils as si

    sdims = ["z", "y", "x"][-image.ndim:]
    spacing = spacing or (1.0,) * image.ndim
    origin = origin or (0.0,) * image.ndim
    sim = si.to_spatial_image(image, dims=sdims, scale=dict(zip(sdims, spacing)), translation=dict(zip(sdims, origin)))
    return msi_utils.get_msim_from_sim(sim)


def _assert_separated(want64, window):
    """The condition under which a float32 computation must reproduce the detections: no near tie inside a window and no
    candidate near the threshold (figures of the float64 restatement)."""
    _, r64, mask64, thr64 = want64
    gaps = do.runner_up_gaps(r64, mask64, window)
    assert mask64.any() and gaps.min() >= 1e-3 * r64.max(), gaps.min() / r64.max()
    assert do.candidate_threshold_margin(r64, window, thr64) >= 0.5


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("icase", range(len(CASES)), ids=CASE_IDS)
def test_log_detect_and_detect_beads_equal_the_oracle(hip_device, icase, dtype, mem):
    from multiview_stitcher_amd import detection

    image, pos, spacing, target, want64, want32 = _case(icase, np.dtype(dtype).name)
    shape, t = CASES[icase]
    _, _, window = do.parameters(spacing, target)
    _assert_separated(want64, window)
    data = _put(image, mem, hip_device)
    labels = detection.log_detect(data, spacing, target, device=hip_device)
    assert labels.dtype == np.int32
    np.testing.assert_array_equal(labels, want32[0])

    origin = (3.0, -2.5, 10.0)[-len(shape):]
    points = detection.detect_beads(_msim(data, origin), detection_func_kwargs={"target_size_physical": target}, device=hip_device)
    want_points = do.label_centroids(want32[0]) + np.asarray(origin)
    assert points.shape == want_points.shape and points.dtype == np.float64
    np.testing.assert_allclose(points, want_points, atol=1e-9, rtol=0)
    diam = np.full(len(shape), float(t)) if np.isscalar(t) else np.asarray(t, dtype=np.float64)
    for p in pos:
        if np.all(p > diam) and np.all(p < np.asarray(shape) - 1 - diam):
            assert np.abs(points - np.asarray(origin) - p).max(axis=1).min() <= 0.75, p


@functools.lru_cache(maxsize=None)
def _slab_case():
    """(32, 36, 44) with a bright slab z in [0, 10): the beads planted inside it have no dark voxel in their neighbourhood."""
    image, pos = do.make_beads((32, 36, 44), (4, 5, 5), seed=5, dtype=np.uint16, slab=(0, 0, 10, 1500.0))
    image.setflags(write=False)
    return image, pos


@pytest.mark.parametrize("neigh_sigma", [None, 1.0], ids=["raw", "smoothed"])
def test_max_neigh_intensity_rejects_the_beads_inside_a_bright_slab(hip_device, neigh_sigma):
    from multiview_stitcher_amd import detection

    image, pos = _slab_case()
    spacing, target = (1.0, 1.0, 1.0), {"z": 4.0, "y": 5.0, "x": 5.0}
    kw = {"max_neigh_intensity": 800.0, "max_neigh_sigma": neigh_sigma}      # (the box is the target size: it reaches past the bead)
    want = do.log_detect(image, spacing, target, **kw)
    plain = do.log_detect(image, spacing, target, mode=np.float64, return_parts=True)
    _assert_separated(plain, do.parameters(spacing, target)[2])
    inside = [p for p in pos if p[0] <= 5]
    outside = [p for p in pos if p[0] >= 17]
    assert inside and outside and 0 < want.max() < plain[0].max()
    got = detection.log_detect(image, spacing, target, device=hip_device, **kw)
    np.testing.assert_array_equal(got, want)
    c = do.label_centroids(got)
    for p in inside:
        assert np.abs(c - p).max(axis=1).min() > 2.0
    for p in outside:
        if np.all(p > 5) and np.all(p < np.asarray(image.shape) - 6):
            assert np.abs(c - p).max(axis=1).min() <= 0.75
    with pytest.raises(ValueError):
        detection.log_detect(image, spacing, target, max_neigh_intensity=800.0, max_neigh_sample_size=0.5, device=hip_device)


def test_threshold_abs(hip_device):
    from multiview_stitcher_amd import detection

    image, _, spacing, target, want64, _ = _case(1, "uint16")
    peaks = np.sort(want64[1][want64[2]])
    thr = float(0.5 * (peaks[len(peaks) // 2 - 1] + peaks[len(peaks) // 2]))      # between the two middle detections
    want = do.log_detect(image, spacing, target, threshold_abs=thr, return_parts=True)
    _, _, window = do.parameters(spacing, target)
    assert 0 < want[0].max() < want64[0].max()
    assert do.candidate_threshold_margin(want64[1], window, thr) >= 1e-3      # (float32 responses differ by 1e-7 of the maximum)
    np.testing.assert_array_equal(detection.log_detect(image, spacing, target, threshold_abs=thr, device=hip_device), want[0])


def test_slabbed_detect_beads_equals_the_unslabbed_call(hip_device):
    """threshold_rel refers to the maximum of the whole field, so three slabs give the points of one block."""
    from multiview_stitcher_amd import detection

    image, _, spacing, target, _, _ = _case(2, "uint16")
    kw = {"target_size_physical": target}
    overlap = detection.log_detect.required_overlap(kw | {"spacing": spacing})[0]
    plane = image.shape[1] * image.shape[2]
    whole = detection.detect_beads(_msim(image), detection_func_kwargs=kw, device=hip_device)
    slabbed = detection.detect_beads(_msim(image), detection_func_kwargs=kw, device=hip_device, max_block_voxels=(11 + 2 * overlap) * plane)
    assert len(detection._slabs(image.shape[0], 11, overlap)) == 3 and len(whole) > 3
    np.testing.assert_array_equal(slabbed, whole)


# ---- 4. context lanes -----------------------------------------------------------------------------------------------------------
def test_two_lanes_at_once_equal_the_serial_results(hip_device):
    from multiview_stitcher_amd import detection

    jobs = [_case(1, "uint16")[:4], _case(0, "float32")[:4]]
    run = lambda job, dev: detection.log_detect(job[0], job[2], job[3], device=dev)      # noqa: E731
    serial = [run(job, hip_device) for job in jobs]
    results, errors = [None, None], []
    barrier = threading.Barrier(2)

    def work(k):
        try:
            barrier.wait(timeout=60)
            for _ in range(3):
                results[k] = run(jobs[k], hip_device | (k + 1) << 8)
        except BaseException as e:          # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for got, want in zip(results, serial):
        assert got.max() > 0
        np.testing.assert_array_equal(got, want)


def test_a_lane_waits_for_an_upload_still_in_flight(hip_device):
    """A tile uploaded asynchronously and detected on lane 1 right away: the lane's stream waits for the copy (a 128 MiB upload
    queued ahead of it keeps the copy stream busy), for the image of the response and for the sample volume of the minimum rule."""
    from multiview_stitcher_amd import detection
    from multiview_stitcher_amd.device import DeviceArray, pinned_empty

    image, _ = do.make_beads((20, 36, 44), (4, 5, 5), seed=77, dtype=np.uint16)      # an image no earlier test left in device memory
    spacing, target = (1.0, 1.0, 1.0), {"z": 4.0, "y": 5.0, "x": 5.0}
    lane = hip_device | 1 << 8
    ballast = pinned_empty((128 << 20,), np.uint8)
    ballast[:] = 1
    staged = pinned_empty(image.shape, image.dtype)
    staged[...] = image
    for kw in ({}, {"max_neigh_intensity": 800.0}):
        want = do.log_detect(image, spacing, target, **kw)
        assert want.max() >= 3
        _assert_separated(do.log_detect(image, spacing, target, mode=np.float64, return_parts=True), do.parameters(spacing, target)[2])
        held = DeviceArray.from_host_async(ballast, hip_device)
        tile = DeviceArray.from_host_async(staged, hip_device)
        assert tile.ready_ticket
        got = detection.log_detect(tile, spacing, target, device=lane, **kw)
        np.testing.assert_array_equal(got, want)
        held.sync_ready()
