"""GPU: registration.masked_correlation_registration (mvs_masked_corr) against the float64 brute force of tests/masked_corr_oracle.py
on the cases of tests/masked_corr_cases.py: peak, overlap counts (exact), r within 8x the error of the float32 restatement, the
sub-pixel shift, every status, determinism, the in-place spectral combine at two padded shapes, and the two public seams."""
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
