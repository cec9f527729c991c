"""GPU: registration.masked_correlation_registration (mvs_masked_corr) against the float64 brute force of tests/masked_corr_oracle.py
on the cases of tests/masked_corr_cases.py: peak, overlap counts (exact), r within 8x the error of the float32 restatement, the
sub-pixel shift, every status, determinism, the in-place spectral combine at two padded shapes, and the two public seams; the same
against the float64 transform oracle on three large cases (several trips of every grid-stride loop, folds of 1024 partials, the long
axes of the transform); and the value edges: infinities, data on a camera offset, valid_above at a voxel's value, mask bytes other
than 1, eligibility at equality, the order of the statuses."""
import warnings

import numpy as np
import pytest

from tests import masked_corr_cases as mc
from tests import masked_corr_oracle as mo

pytestmark = pytest.mark.gpu


def _run(case, hip_device, on_device=False, masks_on_device=False, **overrides):
    from multiview_stitcher_amd import registration
    from multiview_stitcher_amd.device import DeviceArray

    kw = dict(case["kwargs"])
    kw.update(max_shift=case["max_shift"], return_debug=True, device=hip_device)
    kw.update(overrides)
    F, M = case["F"], case["M"]
    if on_device:
        F, M = DeviceArray.from_host(F, hip_device), DeviceArray.from_host(M, hip_device)
    if masks_on_device:
        for k in ("fixed_mask", "moving_mask"):
            if kw.get(k) is not None:
                kw[k] = DeviceArray.from_host(kw[k], hip_device)
    return registration.masked_correlation_registration(F, M, **kw)


@pytest.mark.parametrize("where", ["host", "device", "device_masks"])
@pytest.mark.parametrize("name", list(mc.CASES))
def test_parity_with_the_brute_force(hip_device, name, where):
    """Measured on an MI355X, max |r - brute force| over the eligible shifts (the same for host and resident crops): 4.83e-6,
    8.12e-6, 1.45e-6, 1.35e-6, 6.51e-6, 2.08e-6 in the order of the cases, against a tolerance of 1.76e-5."""
    case, brute, f32 = mc.case_with_oracle(name)
    res = _run(case, hip_device, on_device=where != "host", masks_on_device=where == "device_masks")
    dbg = res["debug"]
    assert dbg["status"] == 0
    assert dbg["peak"] == brute["peak"] == case["offset"]
    assert dbg["padded_shape"] == f32["padded_shape"] and list(dbg["max_shift"]) == brute["shifts"]
    assert dbg["n"].dtype == np.int32 and dbg["r"].dtype == np.float32 and dbg["r"].shape == brute["r"].shape
    assert np.array_equal(dbg["n"], brute["n"])                   # rint of a float32 transform is exact at these sizes
    assert dbg["n_max"] == brute["n_max"] and dbg["n_peak"] == brute["n"][brute["peak_window"]]
    assert dbg["n_valid"] == (int(case["vF"].sum()), int(case["vM"].sum()))
    el = brute["eligible"]
    err = float(np.abs(dbg["r"].astype(np.float64) - brute["r"])[el].max())
    print(name, where, "max |dr| over eligible shifts", err, "restatement", mc.MEASURED_R_ERROR[name], "tolerance", mc.GPU_R_TOLERANCE)
    assert err <= mc.GPU_R_TOLERANCE
    assert np.all(np.abs(dbg["r"]) <= 1.0)
    assert res["quality"] == float(dbg["r"][brute["peak_window"]])
    # sub-pixel: the parabola of the oracle's r, within the r error over the oracle's curvature, times 8
    want, curv = mo.subpixel(brute["r"], el, brute["peak_window"])
    t = res["affine_matrix"][:-1, -1]
    assert np.array_equal(res["affine_matrix"][:-1, :-1], np.eye(len(want)))
    for d, (w, k) in enumerate(zip(want, curv)):
        got = dbg["subpixel"][d]
        assert float(t[d]) == brute["peak"][d] + got
        if np.isnan(k):
            assert got == 0.0
        else:
            assert k < 0
            print("  axis", d, "sub-pixel", got, "oracle", w, "tolerance", 8 * mc.R_ERROR / abs(k))
            assert abs(got - w) <= 8 * mc.R_ERROR / abs(k)
    # without the refinement: the integer peak
    if where == "host":
        plain = _run(case, hip_device, subpixel=False, return_debug=False)
        assert plain["affine_matrix"][:-1, -1].tolist() == [float(p) for p in brute["peak"]] and "debug" not in plain
        assert plain["quality"] == res["quality"]


def _assert_identity(res, ndim):
    assert np.array_equal(res["affine_matrix"], np.eye(ndim + 1)) and np.isnan(res["quality"])


def test_every_status_is_reached_and_warns(hip_device):
    from multiview_stitcher_amd import _lib, registration

    rng = np.random.default_rng(0)
    a, b = rng.random((12, 14)).astype(np.float32), rng.random((12, 14)).astype(np.float32)
    # an all-NaN moving crop
    with pytest.warns(UserWarning, match="fewer than min_overlap"):
        res = registration.masked_correlation_registration(a, np.full_like(b, np.nan), device=hip_device, return_debug=True)
    _assert_identity(res, 2)
    assert res["debug"]["status"] == _lib.MVS_MASKED_CORR_TOO_FEW_VALID == mo.brute_force(a, np.full_like(b, np.nan))["status"]
    assert res["debug"]["n_valid"] == (a.size, 0) and res["debug"]["n_max"] == 0
    # a crop constant on its valid voxels (and not elsewhere)
    m = np.ones(a.shape, np.uint8)
    m[3:, :] = 0
    flat = b.copy()
    flat[:3, :] = 7.0
    with pytest.warns(UserWarning, match="constant"):
        res = registration.masked_correlation_registration(a, flat, moving_mask=m, device=hip_device, return_debug=True)
    _assert_identity(res, 2)
    assert res["debug"]["status"] == _lib.MVS_MASKED_CORR_CONSTANT_CROP == mo.brute_force(a, flat, moving_mask=m)["status"]
    # disjoint masks, no shift of the window brings them together
    left, right = np.zeros(a.shape, np.uint8), np.zeros(a.shape, np.uint8)
    left[:, :6], right[:, 8:] = 1, 1
    with pytest.warns(UserWarning, match="no shift"):
        res = registration.masked_correlation_registration(a, b, fixed_mask=right, moving_mask=left, overlap_ratio=1.0, max_shift=1, device=hip_device,
                                                           return_debug=True)
    _assert_identity(res, 2)
    assert res["debug"]["status"] == _lib.MVS_MASKED_CORR_NO_ELIGIBLE_SHIFT
    assert mo.brute_force(a, b, fixed_mask=right, moving_mask=left, overlap_ratio=1.0, max_shift=1)["status"] == mo.STATUS_NO_ELIGIBLE_SHIFT
    assert res["debug"]["n_max"] == 0 and not res["debug"]["n"].any() and not res["debug"]["r"].any()
    # and the same crops are fine without the masks
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ok = registration.masked_correlation_registration(a, a, subpixel=False, device=hip_device)
    assert ok["affine_matrix"][:-1, -1].tolist() == [0.0, 0.0] and 1.0 - mc.GPU_R_TOLERANCE <= ok["quality"] <= 1.0


@pytest.mark.parametrize("name", ["nan_6x9x11", "above_24x40_shift_5_7"])
def test_two_runs_give_equal_bits(hip_device, name):
    case, _, _ = mc.case_with_oracle(name)
    first, second = _run(case, hip_device), _run(case, hip_device, on_device=True)
    assert first["debug"]["r"].tobytes() == second["debug"]["r"].tobytes()
    assert first["debug"]["n"].tobytes() == second["debug"]["n"].tobytes()
    assert first["affine_matrix"].tobytes() == second["affine_matrix"].tobytes()
    assert np.float64(first["quality"]).tobytes() == np.float64(second["quality"]).tobytes()
    for key in ("peak", "n_peak", "n_max", "n_valid", "padded_shape", "max_shift", "status", "subpixel"):
        assert first["debug"][key] == second["debug"][key], key


# the smaller windows give other padded shapes than the default window of the case
@pytest.mark.parametrize("name, small, small_padded", [
    ("mask_8x16x16", (0, 5, 5), (8, 32, 32)),
    ("mask_8x16x16", (3, 0, 5), (16, 16, 32)),
    ("nan_1x17", (0, 4), (1, 32)),
    ("nan_1x17", (0, 15), (1, 32)),
])
def test_in_place_combine_at_two_padded_shapes(hip_device, name, small, small_padded):
    """The spectral combine works in place on pairs {k, -k}: the same shifts from transforms of another shape agree."""
    case, brute, f32 = mc.case_with_oracle(name)
    full = _run(case, hip_device)["debug"]
    part = _run(case, hip_device, max_shift=small)["debug"]
    assert part["padded_shape"] == small_padded != full["padded_shape"] == f32["padded_shape"]
    S = brute["shifts"]
    shared = tuple(slice(s - k, s + k + 1) for s, k in zip(S, small))
    assert part["r"].shape == full["r"][shared].shape
    assert np.array_equal(part["n"], full["n"][shared]) and np.array_equal(part["n"], brute["n"][shared])
    el = brute["eligible"][shared]
    assert el.any()
    for other in (full["r"][shared].astype(np.float64), brute["r"][shared]):
        assert np.abs(part["r"].astype(np.float64) - other)[el].max() <= mc.GPU_R_TOLERANCE


@pytest.mark.parametrize("where", ["host", "device", "device_masks"])
@pytest.mark.parametrize("name", list(mc.LARGE_CASES))
def test_large_cases_match_the_float64_oracle(hip_device, name, where):
    """The chain where every grid-stride loop makes more than one trip, the folds read more than 256 partials and the transforms
    take their LDS Stockham and four-step paths (tests/test_masked_corr_host.py asserts that the cases get there), against
    ``fft_float64``.  Counts and the peak are exact; r is allowed 8 x the error of the float32 restatement of its case.
    Measured on an MI355X, max |r - fft_float64| over the eligible shifts (the same for host and resident crops): 2.47e-5, 1.10e-5,
    4.49e-6 in the order of the cases, against tolerances of 5.38e-5, 2.30e-5, 9.76e-6."""
    case, oracle, f32 = mc.case_with_oracle(name)
    res = _run(case, hip_device, on_device=where != "host", masks_on_device=where == "device_masks")
    dbg = res["debug"]
    assert dbg["status"] == 0
    assert dbg["peak"] == oracle["peak"] == case["offset"]
    assert dbg["padded_shape"] == oracle["padded_shape"] and list(dbg["max_shift"]) == oracle["shifts"] == list(case["max_shift"])
    assert dbg["n"].dtype == np.int32 and dbg["r"].dtype == np.float32 and dbg["r"].shape == oracle["r"].shape
    differ = np.argwhere(dbg["n"] != oracle["n"])
    if len(differ):
        w = tuple(differ[0])
        print(name, where, len(differ), "counts differ; the first at window index", w, ":", dbg["n"][w], "against", oracle["n"][w],
              "; largest difference", int(np.abs(dbg["n"].astype(np.int64) - oracle["n"]).max()))
    assert len(differ) == 0
    assert dbg["n_max"] == oracle["n_max"] and dbg["n_peak"] == oracle["n"][oracle["peak_window"]]
    assert dbg["n_valid"] == (int(case["vF"].sum()), int(case["vM"].sum()))
    el = oracle["eligible"]
    tolerance = mc.GPU_R_TOLERANCE_LARGE[name]
    err = float(np.abs(dbg["r"].astype(np.float64) - oracle["r"])[el].max())
    print(name, where, "max |dr| over eligible shifts", err, "restatement", mc.MEASURED_R_ERROR_LARGE[name], "tolerance", tolerance)
    assert err <= tolerance
    assert np.all(np.abs(dbg["r"]) <= 1.0)
    assert res["quality"] == float(dbg["r"][oracle["peak_window"]])
    want, curv = mo.subpixel(oracle["r"], el, oracle["peak_window"])
    t = res["affine_matrix"][:-1, -1]
    assert np.array_equal(res["affine_matrix"][:-1, :-1], np.eye(len(want)))
    for d, (w, k) in enumerate(zip(want, curv)):
        got = dbg["subpixel"][d]
        assert float(t[d]) == oracle["peak"][d] + got
        if np.isnan(k):                # (the first axis of nan_3x4100_shift_1_10: the peak lies on the edge of the window)
            assert got == 0.0
        else:
            assert k < 0
            print("  axis", d, "sub-pixel", got, "oracle", w, "tolerance", tolerance / abs(k))
            assert abs(got - w) <= tolerance / abs(k)


def test_large_case_with_the_crops_swapped(hip_device):
    """r of (moving, fixed) at s is r of (fixed, moving) at -s: the oracle's window volumes, reversed.  The peak of
    nan_520x520_shift_300 then lies at window index 150 * 601 + 311 = 90461, which is the partial of workgroup 353: the fold of the
    arg-max partials finds it in its second trip (the peak of the case as it stands is the partial of workgroup 33).
    Measured on an MI355X: max |dr| over the eligible shifts 2.91e-5, against the tolerance of the case, 5.38e-5."""
    name = "nan_520x520_shift_300"
    case, oracle, _ = mc.case_with_oracle(name)
    swapped = dict(case, F=case["M"], M=case["F"], kwargs={"fixed_mask": case["kwargs"]["moving_mask"]})
    dbg = _run(swapped, hip_device)["debug"]
    rev = tuple(slice(None, None, -1) for _ in oracle["r"].shape)
    r, n, el = oracle["r"][rev], oracle["n"][rev], oracle["eligible"][rev]
    assert dbg["status"] == 0 and dbg["peak"] == [-k for k in case["offset"]]
    flat = int(np.ravel_multi_index([s - k for s, k in zip(oracle["shifts"], case["offset"])], r.shape))
    assert flat == 90461 and (flat % mc.ITEMS_PER_TRIP) // 256 == 353 > 256
    assert np.array_equal(dbg["n"], n) and dbg["n_max"] == oracle["n_max"] and dbg["n_peak"] == oracle["n"][oracle["peak_window"]]
    assert dbg["n_valid"] == (int(case["vM"].sum()), int(case["vF"].sum()))
    err = float(np.abs(dbg["r"].astype(np.float64) - r)[el].max())
    print(name, "swapped: max |dr| over eligible shifts", err, "tolerance", mc.GPU_R_TOLERANCE_LARGE[name])
    assert err <= mc.GPU_R_TOLERANCE_LARGE[name]


def test_large_case_gives_equal_bits(hip_device):
    """Folds over 1024 partials in a fixed tree: host crops and resident crops give the same bits."""
    case, _, _ = mc.case_with_oracle("nan_520x520_shift_300")
    first, second = _run(case, hip_device), _run(case, hip_device, on_device=True)
    assert first["debug"]["r"].tobytes() == second["debug"]["r"].tobytes()
    assert first["debug"]["n"].tobytes() == second["debug"]["n"].tobytes()
    assert first["affine_matrix"].tobytes() == second["affine_matrix"].tobytes()
    assert np.float64(first["quality"]).tobytes() == np.float64(second["quality"]).tobytes()
    for key in ("peak", "n_peak", "n_max", "n_valid", "padded_shape", "max_shift", "status", "subpixel"):
        assert first["debug"][key] == second["debug"][key], key


# ---- value edges ---------------------------------------------------------------------------------------------------------------------
def _assert_matches_brute_force(dbg, brute, tolerance, what):
    assert dbg["status"] == brute["status"] == 0 and dbg["peak"] == brute["peak"]
    assert np.array_equal(dbg["n"], brute["n"]) and dbg["n_max"] == brute["n_max"] and dbg["n_peak"] == brute["n"][brute["peak_window"]]
    err = float(np.abs(dbg["r"].astype(np.float64) - brute["r"])[brute["eligible"]].max())
    print(what, "max |dr| over eligible shifts", err, "tolerance", tolerance)
    assert err <= tolerance


def test_infinities_are_not_valid(hip_device):
    case, brute, _ = mc.value_case("inf")
    dbg = _run(case, hip_device)["debug"]
    assert dbg["n_valid"] == (int(case["vF"].sum()), int(case["vM"].sum()))
    _assert_matches_brute_force(dbg, brute, mc.GPU_R_TOLERANCE, "infinities:")
    assert brute["peak"] == case["offset"] and np.all(np.isfinite(dbg["r"]))


def test_camera_offset_is_centred_away(hip_device):
    """Whole numbers of an amplitude of about 50 around 30000: without the centring of the pack pass the variance sums would cancel
    in float32 (the float32 restatement without it is off by 0.89, tests/test_masked_corr_host.py).  The GPU is allowed 8 x the
    error of the restatement with it, 1.57e-5.  Measured on an MI355X: 5.75e-6."""
    case, brute, _ = mc.value_case("camera")
    dbg = _run(case, hip_device)["debug"]
    assert dbg["n_valid"] == (int(case["vF"].sum()), int(case["vM"].sum()))
    _assert_matches_brute_force(dbg, brute, 8 * mc.MEASURED_R_ERROR_CAMERA, "camera offset:")
    assert brute["peak"] == case["offset"]


@pytest.mark.parametrize("exact", [False, True])
def test_valid_above_at_a_value(hip_device, exact):
    """Voxels of float32(0.1): valid above the double 0.1 (the comparison is made in double), not above float32(0.1) itself."""
    thr = float(mc.THRESHOLD_VALUE) if exact else 0.1
    case, brute, _ = mc.value_case("threshold", valid_above=(thr, thr))
    dbg = _run(case, hip_device)["debug"]
    at_value = [(case[im] == mc.THRESHOLD_VALUE) for im in ("F", "M")]
    n_valid = tuple(int(mo.validity(case[im], None, thr).sum()) for im in ("F", "M"))
    assert dbg["n_valid"] == n_valid
    assert all((mo.validity(case[im], None, thr) & m).sum() == (0 if exact else m.sum()) for im, m in zip(("F", "M"), at_value))
    _assert_matches_brute_force(dbg, brute, mc.GPU_R_TOLERANCE, f"valid_above={thr!r}:")
    # a scalar threshold is the pair of it
    assert _run(case, hip_device, valid_above=thr)["debug"]["n"].tobytes() == dbg["n"].tobytes()


def test_any_non_zero_mask_byte_counts(hip_device):
    case, _, _ = mc.case_with_oracle("mask_8x16x16")
    ones = _run(case, hip_device)["debug"]
    for value in (2, 128, 255):
        masks = {k: (case["kwargs"][k] * np.uint8(value)).astype(np.uint8) for k in ("fixed_mask", "moving_mask")}
        assert all(set(np.unique(m)) == {0, value} for m in masks.values())
        for on_device in (False, True):
            other = _run(case, hip_device, masks_on_device=on_device, **masks)["debug"]
            assert other["r"].tobytes() == ones["r"].tobytes() and other["n"].tobytes() == ones["n"].tobytes(), value
            assert other["n_valid"] == ones["n_valid"] and other["peak"] == ones["peak"]


def test_eligibility_at_equality(hip_device):
    """N at the planted shift is 64 = 0.5 max N exactly: eligible (>=) and the peak; at overlap_ratio 0.51 it is not."""
    for ratio in (0.5, 0.51):
        case, brute, _ = mc.value_case("eligibility", overlap_ratio=ratio)
        dbg = _run(case, hip_device)["debug"]
        planted = tuple(k + s for k, s in zip(case["offset"], brute["shifts"]))
        assert dbg["n"][planted] == 64 and dbg["n_max"] == 128
        _assert_matches_brute_force(dbg, brute, mc.GPU_R_TOLERANCE, f"overlap_ratio={ratio}:")
        assert (dbg["peak"] == case["offset"]) == (ratio == 0.5) == bool(brute["eligible"][planted])


def test_too_few_valid_comes_before_constant(hip_device):
    from multiview_stitcher_amd import _lib, registration

    rng = np.random.default_rng(2)
    a, b = rng.random((12, 14)).astype(np.float32), rng.random((12, 14)).astype(np.float32)
    three = np.full_like(b, np.nan)
    three[4, 3:6] = 7.0                # three valid voxels, all equal
    with pytest.warns(UserWarning, match="fewer than min_overlap"):
        res = registration.masked_correlation_registration(a, three, device=hip_device, return_debug=True)
    assert res["debug"]["status"] == _lib.MVS_MASKED_CORR_TOO_FEW_VALID == mo.brute_force(a, three)["status"]
    assert res["debug"]["n_valid"] == (a.size, 3)
    sixteen = np.full_like(b, np.nan)
    sixteen[2:6, 5:9] = b[2:6, 5:9]    # min_overlap = 4 ** 2 valid voxels exactly, not constant
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = registration.masked_correlation_registration(a, sixteen, device=hip_device, return_debug=True)
    want = mo.brute_force(a, sixteen)
    assert res["debug"]["n_valid"] == (a.size, 16) and res["debug"]["status"] == want["status"] == _lib.MVS_MASKED_CORR_OK
    assert res["debug"]["peak"] == want["peak"] and np.array_equal(res["debug"]["n"], want["n"])
    fifteen = sixteen.copy()
    fifteen[2, 5] = np.nan
    with pytest.warns(UserWarning, match="fewer than min_overlap"):
        res = registration.masked_correlation_registration(a, fifteen, device=hip_device, return_debug=True)
    assert res["debug"]["status"] == _lib.MVS_MASKED_CORR_TOO_FEW_VALID and res["debug"]["n_valid"] == (a.size, 15)


def test_through_dispatch_pairwise_reg_func(hip_device):
    from multiview_stitcher_amd import registration

    case, brute, _ = mc.case_with_oracle("nan_13x20")
    direct = _run(case, hip_device, return_debug=False)
    via = registration.dispatch_pairwise_reg_func(registration.masked_correlation_registration, fixed_data=case["F"], moving_data=case["M"],
                                                  device=hip_device, max_shift=case["max_shift"], **case["kwargs"])
    assert via["affine_matrix"].tobytes() == direct["affine_matrix"].tobytes() and via["quality"] == direct["quality"]
    assert np.round(via["affine_matrix"][:-1, -1]).tolist() == [float(p) for p in brute["peak"]]


def test_through_register_on_a_two_tile_mosaic(hip_device):
    """register() with the masked correlation as pairwise_reg_func and the acquisition's Otsu threshold as valid_above recovers the
    hidden offset to within 0.5 px of what the phase correlation finds on the same mosaic."""
    from multiview_stitcher_amd import masks, param_utils, registration, sample_data
    from tests.helpers import squeeze_field

    key = sample_data.METADATA_TRANSFORM_KEY
    shifts = {}
    for which in ("phase", "masked"):
        sims, jit, _ = sample_data.generate_tiled_dataset(ndim=2, tile_shape=(96, 128), tiles=(1, 2), overlap=(0, 32), max_jitter=3, seed=11)
        assert np.abs(jit[1]).max() > 0
        kwargs = {}
        if which == "masked":
            threshold = masks.otsu_threshold([squeeze_field(s) for s in sims], device=hip_device)
            kwargs = dict(pairwise_reg_func=registration.masked_correlation_registration, pairwise_reg_func_kwargs={"valid_above": threshold})
        res = registration.register(sims, transform_key=key, new_transform_key="reg", reg_channel_index=0, device=hip_device,
                                    groupwise_resolution_kwargs={"reference_view": 0}, return_dict=True, **kwargs)
        got = np.array([param_utils.select_time(p, 0)[:-1, -1] for p in res["params"]])
        shifts[which] = got[1] - got[0]
        print(which, "shift of tile 1 against tile 0", shifts[which], "hidden", jit[1] - jit[0])
    # (measured on an MI355X: hidden (3, 3), phase correlation (2.9, 2.7), masked correlation (3.0006, 2.9861))
    assert np.abs(shifts["masked"] - shifts["phase"]).max() <= 0.5
    assert np.abs(shifts["masked"] - (jit[1] - jit[0])).max() <= 0.5
