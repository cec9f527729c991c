"""CPU: the host side of the bead detection -- sparse labelling and centroids against scipy.ndimage, the filter taps against
scipy's line filter, the index arithmetic of csrc/mvs_detect_dev.h compiled for the host, the parameter derivation against values
worked out by hand, and the detect_beads driver with the two device operations replaced by the scipy restatement
(tests/detection_oracle.py): level choice, origin and spacing, custom detection functions, slabs."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from multiview_stitcher_amd import _detect_ops, detection, msi_utils
from multiview_stitcher_amd import spatial_image_utils as si
from tests import detection_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- sparse labelling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.02, 0.3, 0.7])
@pytest.mark.parametrize("shape", [(17, 70), (5, 6, 7), (3, 4, 130)], ids=str)
def test_sparse_labels_and_centroids_equal_scipy(shape, density):
    mask = np.random.default_rng(int(1000 * density) + sum(shape)).random(shape) < density
    want, n = ndimage.label(mask)
    coords = np.argwhere(mask)
    labels = detection.label_sparse(coords, shape)
    assert labels.dtype == np.int32 and n >= 1
    np.testing.assert_array_equal(labels, want[mask])
    want_c = np.asarray(ndimage.center_of_mass(want, want, np.arange(1, n + 1)))
    np.testing.assert_allclose(detection.sparse_centroids(coords, labels), want_c, atol=1e-12, rtol=0)


@pytest.mark.parametrize("shape", [(17, 70), (5, 6, 7)], ids=str)
def test_an_empty_mask_gives_no_points(shape):
    coords = np.argwhere(np.zeros(shape, bool))
    labels = detection.label_sparse(coords, shape)
    assert labels.shape == (0,)
    assert detection.sparse_centroids(coords, labels).shape == (0, len(shape))
    with pytest.raises(ValueError):
        detection.label_sparse(np.array([[1, 2], [1, 1]]), (4, 5))


# ---- filter taps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("sigma", [0.5, 1.7, 4.0])
def test_taps_equal_scipys_line_filter(sigma, order):
    radius, taps = _detect_ops.gaussian_taps(sigma, order)
    assert radius == int(4 * sigma + 0.5) and taps.shape == (2 * radius + 1,) and taps.dtype == np.float64
    impulse = np.zeros(4 * radius + 5)
    impulse[2 * radius + 2] = 1.0
    want = ndimage.gaussian_filter1d(impulse, sigma, order=order, mode="constant")[radius + 2:3 * radius + 3]
    np.testing.assert_allclose(taps, want, atol=1e-15, rtol=0)
    if order == 0:
        assert abs(taps.sum() - 1.0) < 1e-15


# ---- mvs_detect_dev.h on the host -------------------------------------------------------------------------------------------------
def test_header_indices_equal_numpy(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "detect_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "detect_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("R ")]
    assert len(rows) == 4 * 81
    for length in (1, 2, 3, 7):
        padded = np.pad(np.arange(length), 40, mode="symmetric")          # padded[p + 40] = source index of position p
        got = {p: q for n, p, q in rows if n == length}
        assert sorted(got) == list(range(-40, 41))
        for p in range(-40, 41):
            assert got[p] == padded[p + 40], (length, p)
    wins = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("W ")]
    assert len(wins) == 6 * 5
    ramp = np.arange(21)
    for n, i, lo, hi in wins:
        assert (lo, hi) == (i - n // 2, i - n // 2 + n - 1)
        # scipy's rank filters read exactly these samples
        assert ndimage.minimum_filter1d(ramp, n)[i] == lo and ndimage.maximum_filter1d(ramp, n)[i] == hi


# ---- parameters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,target,sigma,window,overlap", [
    ((1.0, 1.0), 5.0, (1.7677669529663689,) * 2, (7, 7), (10, 10)),                        # 5 / (2 sqrt 2); ceil(7.071 + 2.5)
    ((0.5, 0.5, 0.5), 3.0, (1.7320508075688772,) * 3, (7, 7, 7), (10, 10, 10)),            # 6 px: sqrt 3; ceil(6.928 + 3)
    ((2.0, 0.5, 0.5), {"z": 4.0, "y": 2.0, "x": 2.0}, (0.5773502691896258, 1.1547005383792517, 1.1547005383792517), (3, 5, 5), (4, 7, 7)),
    ((4.0, 1.0, 1.0), 2.0, (0.5, 0.5773502691896258, 0.5773502691896258), (3, 3, 3), (3, 4, 4)),   # sigma floor along z
], ids=["2d", "3d", "anisotropic", "floor"])
def test_parameters_and_required_overlap(spacing, target, sigma, window, overlap):
    got_sigma, got_dist, got_window = detection.log_detect_parameters(spacing, target)
    np.testing.assert_allclose(got_sigma, sigma, rtol=1e-15)
    assert got_window == window
    assert all(d >= 1.0 for d in got_dist)
    assert detection.log_detect.required_overlap({"spacing": spacing, "target_size_physical": target}) == overlap
    assert do.parameters(spacing, target)[0] == got_sigma and do.parameters(spacing, target)[2] == got_window
    with pytest.raises(TypeError):
        detection.log_detect_parameters(spacing, True)
    with pytest.raises(TypeError):
        detection.log_detect_parameters(spacing, {"y": 1.0})


def test_neighbourhood_sizes_truncate_like_scipy():
    assert detection._neighbourhood_rule((1.0, 0.5), 2.7, None, None, 2) == ((2, 5), None)
    assert detection._neighbourhood_rule((1.0, 0.5), 2.7, {"y": 3.0, "x": 3.9}, 1.0, 2) == ((3, 7), (1.0, 2.0))
    with pytest.raises(ValueError):
        detection._neighbourhood_rule((1.0, 4.0), 2.7, None, None, 2)


# ---- the driver -----------------------------------------------------------------------------------------------------------------
class StandIn:
    """The two device operations (and the memory question) answered by the restatement; records what it was asked."""

    def __init__(self):
        self.responses, self.maxima = [], []

    def log_response(self, image, sigmas, scale, max_range=None, device=0):
        image = np.asarray(image)
        assert scale == float(np.mean(sigmas)) ** 2
        r = do.response(image, sigmas, np.float32)
        lo, hi = (0, image.shape[0]) if max_range is None else max_range
        self.responses.append({"shape": image.shape, "sigmas": tuple(sigmas), "max_range": max_range})
        return r, r[lo:hi].max()

    def local_maxima(self, response, window, threshold, sample=None, sample_window=None, bound=None, device=0, capacity=None):
        assert sample is None
        self.maxima.append({"shape": response.shape, "window": tuple(window), "threshold": threshold})
        return np.argwhere(do.detections(response, window, np.float32(threshold)))

    def fits_device(self, n_voxels, itemsize, on_host, device=0):
        return True


@pytest.fixture
def stand_in(monkeypatch):
    rec = StandIn()
    for name in ("log_response", "local_maxima", "fits_device"):
        monkeypatch.setattr(_detect_ops, name, getattr(rec, name))
    return rec


def _sim(image, spacing, origin, dims=None):
    sdims = ["z", "y", "x"][-len(spacing):]
    return si.to_spatial_image(image, dims=dims or sdims, scale=dict(zip(sdims, spacing)), translation=dict(zip(sdims, origin)))


BEADS = {}


def _beads(shape, diameter, seed):
    key = (shape, diameter, seed)
    if key not in BEADS:
        image, pos = do.make_beads(shape, diameter, seed)
        image.setflags(write=False)
        BEADS[key] = (image, pos)
    return BEADS[key]


def test_origin_and_spacing_are_applied(stand_in):
    image, _ = _beads((20, 36, 44), (4, 5, 5), 3)
    spacing, origin = (2.0, 0.5, 0.5), (10.0, -3.0, 7.25)
    target = {"z": 8.0, "y": 2.5, "x": 2.5}
    points = detection.detect_beads(msi_utils.get_msim_from_sim(_sim(image, spacing, origin)), detection_func_kwargs={"target_size_physical": target})
    want = do.label_centroids(do.log_detect(image, spacing, target))
    assert len(want) >= 4 and points.dtype == np.float64
    np.testing.assert_allclose(points, np.asarray(origin) + want * np.asarray(spacing), atol=1e-12, rtol=0)
    assert [c["shape"] for c in stand_in.responses] == [image.shape] and stand_in.responses[0]["max_range"] is None
    np.testing.assert_allclose(stand_in.responses[0]["sigmas"], do.parameters(spacing, target)[0])
    labels = detection.log_detect(image, spacing, target)
    np.testing.assert_array_equal(labels, do.log_detect(image, spacing, target))


def test_level_choice_and_first_field(stand_in):
    image, _ = _beads((24, 40, 48), 6, 4)
    two = np.stack([image, np.zeros_like(image)])                  # c = 0 holds the beads
    sim = _sim(two, (1.0, 1.0, 1.0), (0.0, 5.0, -5.0), dims=["c", "z", "y", "x"])
    msim = msi_utils.get_msim_from_sim(sim, scale_factors=[2])
    kw = {"target_size_physical": 6.0}
    level0 = si.get_sim_field(msi_utils.get_sim_from_msim(msim, "scale0"))
    level1 = si.get_sim_field(msi_utils.get_sim_from_msim(msim, "scale1"))
    assert level1.shape == (12, 20, 24) and si.get_spacing_from_sim(level1) == {"z": 2.0, "y": 2.0, "x": 2.0}
    for request, level in ((None, level0), (1.5, level0), (2.5, level1), ({"z": 8.0, "y": 2.0, "x": 2.0}, level1), ({"x": 1.9}, level0)):
        stand_in.responses.clear()
        points = detection.detect_beads(msim, detection_func_kwargs=kw, max_detection_spacing=request)
        assert [c["shape"] for c in stand_in.responses] == [level.shape]
        sp = si.get_spacing_from_sim(level, asarray=True)
        want = do.label_centroids(do.log_detect(np.asarray(level.data), tuple(sp), 6.0))
        assert len(want) >= 3
        np.testing.assert_allclose(points, si.get_origin_from_sim(level, asarray=True) + want * sp, atol=1e-12, rtol=0)


def test_custom_detection_function(stand_in):
    image, _ = _beads((20, 36, 44), (4, 5, 5), 3)
    spacing, origin = (2.0, 1.0, 1.0), (1.0, 2.0, 3.0)
    seen = []

    def bright(block, block_spacing, level):
        seen.append((type(block), block.shape, block_spacing))
        return ndimage.label(block > level)[0].astype(np.int32)

    msim = msi_utils.get_msim_from_sim(_sim(image, spacing, origin))
    points = detection.detect_beads(msim, detection_func=bright, detection_func_kwargs={"level": 1200})
    assert seen == [(np.ndarray, image.shape, spacing)] and not stand_in.responses and not stand_in.maxima
    want = do.label_centroids(ndimage.label(image > 1200)[0])
    assert len(want) >= 4
    np.testing.assert_allclose(points, np.asarray(origin) + want * np.asarray(spacing), atol=1e-12, rtol=0)
    with pytest.raises(TypeError):
        detection.detect_beads(msim, detection_func=lambda block, block_spacing: (block > 1200).astype(np.float32))
    with pytest.raises(TypeError):
        detection.detect_beads(msim, detection_func=bright, detection_func_kwargs={"level": 1200}, detection_overlap=1.5)
    # slabs of a custom function: every object whose centroid lies in a core is reported once
    slabbed = detection.detect_beads(msim, detection_func=bright, detection_func_kwargs={"level": 1200}, detection_overlap=6,
                                     max_block_voxels=(7 + 12) * 36 * 44)
    assert len(seen) == 4 and seen[2][1] == (19, 36, 44)
    assert sorted(map(tuple, np.round(slabbed, 9))) == sorted(map(tuple, np.round(points, 9)))


@pytest.mark.parametrize("threshold", ["abs", "rel"])
def test_three_slabs_give_the_points_of_one_block(stand_in, threshold):
    """With threshold_abs (and, by the documented departure, with threshold_rel) the slab grid does not change the result.  The
    field holds beads whose centroids lie where two slabs overlap: each appears once."""
    image, _ = _beads((33, 31, 29), (6, 3, 3), 31)
    spacing, target = (1.0, 1.0, 1.0), {"z": 6.0, "y": 3.0, "x": 3.0}
    kw = {"target_size_physical": target}
    if threshold == "abs":
        kw["threshold_abs"] = float(0.2 * do.response(image, do.parameters(spacing, target)[0]).max())
    msim = msi_utils.get_msim_from_sim(_sim(image, spacing, (0.0, 0.0, 0.0)))
    whole = detection.detect_beads(msim, detection_func_kwargs=kw)
    assert [c["shape"] for c in stand_in.responses] == [image.shape]
    stand_in.responses.clear()
    stand_in.maxima.clear()
    overlap = detection.log_detect.required_overlap(kw | {"spacing": spacing})[0]
    assert overlap == 10
    slabbed = detection.detect_beads(msim, detection_func_kwargs=kw, max_block_voxels=(11 + 2 * overlap) * 31 * 29)
    slab_shapes = [(21, 31, 29), (31, 31, 29), (21, 31, 29)]
    assert [c["shape"] for c in stand_in.maxima] == slab_shapes
    if threshold == "rel":      # a first sweep for the maximum of the whole field, each slab restricted to its core
        assert [c["max_range"] for c in stand_in.responses[:3]] == [(0, 11), (10, 21), (10, 21)]
        assert len({float(c["threshold"]) for c in stand_in.maxima}) == 1
    else:
        assert [c["shape"] for c in stand_in.responses] == slab_shapes
    assert len(whole) >= 8 and len(np.unique(np.round(whole, 6), axis=0)) == len(whole)
    np.testing.assert_array_equal(slabbed, whole)
    z = whole[:, 0]
    assert ((z >= 1) & (z < 11)).any() and ((z >= 12) & (z < 22)).any()      # in slab 0's core and slab 1's halo; slab 1's core and slab 2's halo
    np.testing.assert_allclose(whole, do.label_centroids(do.log_detect(image, spacing, target)), atol=1e-12, rtol=0)


def test_slab_sizing_stays_within_the_budget_or_says_why_not(stand_in, monkeypatch):
    """No slab is larger than what was asked for or found to fit; a budget below the thinnest slab (one core plane plus the
    overlap on both sides) is refused with a message, not tried."""
    image, _ = _beads((33, 31, 29), (6, 3, 3), 31)
    plane = 31 * 29
    kw = {"target_size_physical": {"z": 6.0, "y": 3.0, "x": 3.0}}
    msim = msi_utils.get_msim_from_sim(_sim(image, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))
    whole = detection.detect_beads(msim, detection_func_kwargs=kw)
    with pytest.raises(ValueError, match="thinnest slab"):
        detection.detect_beads(msim, detection_func_kwargs=kw, max_block_voxels=20 * plane)          # 2 * 10 + 1 planes are needed
    stand_in.maxima.clear()
    thin = detection.detect_beads(msim, detection_func_kwargs=kw, max_block_voxels=21 * plane + 5)
    assert len(stand_in.maxima) == 33 and max(c["shape"][0] for c in stand_in.maxima) == 21
    np.testing.assert_array_equal(thin, whole)
    # without max_block_voxels the device decides: the thickest slab that fits
    asked = []

    def fits(n_voxels, itemsize, on_host, device=0):
        asked.append(n_voxels)
        return n_voxels <= 26 * plane + 7

    monkeypatch.setattr(_detect_ops, "fits_device", fits)
    stand_in.maxima.clear()
    auto = detection.detect_beads(msim, detection_func_kwargs=kw)
    assert asked[0] == image.size and max(c["shape"][0] for c in stand_in.maxima) == 26
    np.testing.assert_array_equal(auto, whole)
    monkeypatch.setattr(_detect_ops, "fits_device", lambda n_voxels, itemsize, on_host, device=0: n_voxels < 21 * plane)
    with pytest.raises(MemoryError, match="thinnest slab"):
        detection.detect_beads(msim, detection_func_kwargs=kw)
