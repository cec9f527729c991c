"""CPU: the masked correlation (registration.masked_correlation_registration) without a device: conditions on the test cases that
the oracle alone checks (of the large cases: every edge of the launch geometry they are there to cross), the float64 transform
oracle of the large cases against the brute force, the float32 restatement of the device chain against both (it sizes the GPU tolerances),
csrc/mvs_masked_corr_plan.h compiled for the host under the address and undefined-behaviour sanitizers, the refusals that need no
device and the sub-pixel parabola."""
import ctypes as C
import hashlib
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _masked_corr_ops as ops, registration
from tests import masked_corr_cases as mc
from tests import masked_corr_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEASURED_R_ERROR, R_ERROR = mc.MEASURED_R_ERROR, mc.R_ERROR


def _far_from(peak_w, shape):
    d = np.max(np.abs(np.indices(shape) - np.array(peak_w).reshape((-1,) + (1,) * len(shape))), axis=0)
    return d > 1


@pytest.mark.parametrize("name", list(mc.CASES))
def test_cases_meet_their_conditions(name):
    """By the oracle alone: the brute-force peak is the planted offset and stands out by at least 0.1 from every eligible shift
    outside its 3^ndim neighbourhood; the windows hold ineligible shifts with |r| = 1 (overlaps of two voxels: the reason for the
    overlap rule) except where max_shift keeps every shift eligible; without masks the zero-filled wedge cases peak elsewhere."""
    case, brute, _ = mc.case_with_oracle(name)
    assert brute["status"] == mo.STATUS_OK
    assert brute["peak"] == case["offset"]
    r, eligible = brute["r"], brute["eligible"]
    far = eligible & _far_from(brute["peak_window"], r.shape)
    assert far.any()
    margin = r[brute["peak_window"]] - r[far].max()
    print(name, "peak r", r[brute["peak_window"]], "margin", margin)
    assert margin >= 0.1
    if name == "above_24x40_shift_5_7":
        assert eligible.all()
    else:
        assert np.abs(r[~eligible]).max() >= 1.0 - 1e-9
    if name in mc.WEDGE_CASES:
        kw = {"min_overlap": case["kwargs"]["min_overlap"]} if "min_overlap" in case["kwargs"] else {}
        assert mo.unmasked_peak(case["F"], case["M"], case["vF"], case["vM"], max_shift=case["max_shift"], **kw) != case["offset"]
    # the validity the case intends is the validity the keyword arguments give
    va = case["kwargs"].get("valid_above", (None, None))
    assert np.array_equal(mo.validity(case["F"], case["kwargs"].get("fixed_mask"), va[0]), case["vF"])
    assert np.array_equal(mo.validity(case["M"], case["kwargs"].get("moving_mask"), va[1]), case["vM"])
    assert np.isfinite(case["M"][~case["vM"]]).any() and np.nanmax(case["M"][~case["vM"]]) == mc.BRIGHT      # the bright block


@pytest.mark.parametrize("name", list(mc.CASES))
def test_float32_restatement_matches_brute_force(name):
    case, brute, f32 = mc.case_with_oracle(name)
    assert f32["peak"] == brute["peak"] and f32["status"] == brute["status"]
    assert np.array_equal(f32["n"], brute["n"]) and f32["n_max"] == brute["n_max"]
    assert np.array_equal(f32["eligible"], brute["eligible"])
    err = float(np.abs(f32["r"].astype(np.float64) - brute["r"])[brute["eligible"]].max())
    print(name, "max |dr| over eligible shifts", err)
    assert err <= 2.0 * MEASURED_R_ERROR[name]
    assert max(MEASURED_R_ERROR.values()) <= R_ERROR
    assert f32["padded_shape"] == ops.padded_shape(case["F"].shape, brute["shifts"])


# sha256 over F, M, vF, vM and the keyword arguments of the six small cases, taken before make_case got its per-case margin
CASE_DIGESTS = {
    "nan_13x20": "ed19011286f78d1c9f3aa4e4cc759f42e7e3a6a3f13414afb60f7f45ac3b4a7e",
    "nan_6x9x11": "7097918fca3a3f06c83cacad50673a51b3042725359d4ccb866e5375ba1dd0df",
    "above_24x40_shift_5_7": "3993fdc9794d9fdee81d60dacdddd712e1d68945f2460242740b37cbe1f37b3b",
    "nan_1x17": "ebcf5d2cc96cf2d15abbd4d3cd847617367688a43844778ab14ca96db54fba2d",
    "mask_8x16x16": "31db97a98439892ab074f07ba7d8d286823cc3e7f089eca24ca1ac763c28c7e7",
    "nan_5x31_edge": "3f5f993d1ca6e74bc5ccb9e4c7d2d4c90f740ea652e109a935c96b43e4431ddd",
}


@pytest.mark.parametrize("name", list(mc.CASES))
def test_small_cases_are_the_arrays_they_were(name):
    """The margin of the field around the crops became per-case for the large offsets; the small cases keep theirs, byte for byte."""
    c = mc.make_case(name)
    h = hashlib.sha256()
    for a in (c["F"], c["M"], c["vF"], c["vM"]):
        h.update(np.ascontiguousarray(a).tobytes())
    for k in sorted(c["kwargs"]):
        v = c["kwargs"][k]
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    assert h.hexdigest() == CASE_DIGESTS[name]
    assert list(mc.CASES) == list(CASE_DIGESTS)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_fft_float64_matches_brute_force(name):
    """The oracle of the large cases against the definition where both can run: every shift of the six small cases.  1e-12 is a
    bound on float64 rounding (measured: 2e-16 .. 8e-16)."""
    case, brute, _ = mc.case_with_oracle(name)
    kw = dict(case["kwargs"])
    kw.setdefault("valid_above", (None, None))
    fft = mo.fft_float64(case["F"], case["M"], max_shift=case["max_shift"], **kw)
    assert np.array_equal(fft["n"], brute["n"]) and fft["n_max"] == brute["n_max"]
    assert np.array_equal(fft["eligible"], brute["eligible"])
    assert fft["peak"] == brute["peak"] and fft["peak_window"] == brute["peak_window"] and fft["status"] == brute["status"]
    assert fft["shifts"] == brute["shifts"] and fft["padded_shape"] == ops.padded_shape(case["F"].shape, brute["shifts"])
    err = float(np.abs(fft["r"] - brute["r"])[brute["eligible"]].max())
    print(name, "max |r(fft_float64) - r(brute force)| over eligible shifts", err)
    assert err <= 1e-12
    assert fft["den"].shape == fft["r"].shape and fft["tol"] == 1e3 * mo.FLT_EPS * fft["den"].max()


def test_brute_force_at_is_the_body_of_brute_force():
    case, brute, _ = mc.case_with_oracle("nan_6x9x11")
    S = brute["shifts"]
    shifts = [(0, 0, 0), (-5, 8, -10), (5, -8, 10), tuple(case["offset"])]
    n, num, den = mo.brute_force_at(case["F"], case["M"], shifts, **case["kwargs"])
    for k, s in enumerate(shifts):
        w = tuple(a + b for a, b in zip(s, S))
        assert n[k] == brute["n"][w]
        if brute["eligible"][w]:
            assert num[k] / den[k] == brute["r"][w]


def _sampled_shifts(oracle, seed):
    """The peak, its 2 ndim axis neighbours, the 2^ndim corners of the window, the zero shift and 256 seeded shifts."""
    S, peak = oracle["shifts"], oracle["peak"]
    ndim = len(S)
    shifts = [tuple(peak), (0,) * ndim]
    for d in range(ndim):
        for step in (-1, 1):
            q = list(peak)
            q[d] += step
            if abs(q[d]) <= S[d]:
                shifts.append(tuple(q))
    shifts += list(itertools.product(*[(-s, s) for s in S]))
    rng = np.random.default_rng(seed)
    shifts += [tuple(int(rng.integers(-s, s + 1)) for s in S) for _ in range(256)]
    return shifts


@pytest.mark.parametrize("name", list(mc.LARGE_CASES))
def test_fft_float64_matches_the_definition_at_sampled_shifts(name):
    case, oracle, _ = mc.case_with_oracle(name)
    S = oracle["shifts"]
    shifts = _sampled_shifts(oracle, seed=11)
    assert len(shifts) <= 300
    n, num, den = mo.brute_force_at(case["F"], case["M"], shifts, **case["kwargs"])
    w = tuple(np.array([[k + s for k, s in zip(shift, S)] for shift in shifts]).T)
    assert np.array_equal(n, oracle["n"][w])
    el = oracle["eligible"][w]
    assert el.sum() >= 200 and np.all(den[el] > 0)
    err = float(np.abs(num[el] / den[el] - oracle["r"][w][el]).max())
    print(name, len(shifts), "shifts,", int(el.sum()), "eligible: max |num / den - r(fft_float64)|", err)
    assert err <= 1e-12


def _trips(items, blocks):
    """Trips of ``for (i = block * 256 + thread; i < items; i += blocks * 256)`` that some thread makes."""
    return -(-items // (blocks * 256))


# voxels, padded, window; blocks of the three grids (= the partials that the statistics and the window folds read); the axes of the
# transform by the kernel that takes them: register (<= 256 points), LDS Stockham (512 .. 4096), four-step (above)
LARGE_GEOMETRY = {
    "nan_520x520_shift_300": dict(items=(270400, 1 << 20, 361201), blocks=(1024, 1024, 1024), trips=(2, 4, 2), padded_shape=(1024, 1024)),
    "nan_20x130x130_shift_3_40_40": dict(items=(338000, 1 << 21, 45927), blocks=(1024, 1024, 180), trips=(2, 8, 1), padded_shape=(32, 256, 256)),
    "nan_3x4100_shift_1_10": dict(items=(12300, 1 << 15, 63), blocks=(49, 128, 1), trips=(1, 1, 1), padded_shape=(4, 8192)),
}


@pytest.mark.parametrize("name", list(mc.LARGE_CASES))
def test_large_cases_meet_their_conditions(name):
    """By the oracle and the float32 restatement alone, so that the GPU test cannot hide a failure: each large case crosses the edges
    it is there for, its peak stands out by 100 x the GPU tolerance, no eligible shift is near the zeroing rule, and rint(N) has room."""
    case, oracle, f32 = mc.case_with_oracle(name)
    shape, S = case["F"].shape, oracle["shifts"]
    geo = LARGE_GEOMETRY[name]
    # the edges: items and blocks of the three grids, trips of their loops, partials against the 256 threads that fold them
    blocks = lambda items: min(max((items + 255) // 256, 1), 1024)
    voxels, padded, window = int(np.prod(shape)), int(np.prod(oracle["padded_shape"])), int(np.prod([2 * s + 1 for s in S]))
    assert (voxels, padded, window) == geo["items"] and oracle["padded_shape"] == geo["padded_shape"] == f32["padded_shape"]
    assert tuple(blocks(v) for v in geo["items"]) == geo["blocks"]
    assert tuple(_trips(v, b) for v, b in zip(geo["items"], geo["blocks"])) == geo["trips"]
    assert list(S) == list(case["max_shift"]) and oracle["r"].shape == tuple(2 * s + 1 for s in S)
    if name == "nan_520x520_shift_300":
        assert voxels > mc.ITEMS_PER_TRIP and padded > mc.ITEMS_PER_TRIP and window > mc.ITEMS_PER_TRIP
        assert geo["blocks"][0] > 256 and geo["blocks"][2] > 256           # a second trip of every fold of partials
        assert all(512 <= p <= 4096 for p in oracle["padded_shape"])       # the LDS Stockham transform on both axes
        flat = int(np.ravel_multi_index(oracle["peak_window"], oracle["r"].shape))
        assert flat == 450 * 601 + 289 and flat >= mc.ITEMS_PER_TRIP       # a thread finds the peak in its second trip
    elif name == "nan_20x130x130_shift_3_40_40":
        assert voxels > mc.ITEMS_PER_TRIP and padded == 8 * mc.ITEMS_PER_TRIP and window <= mc.ITEMS_PER_TRIP
        assert geo["blocks"][0] > 256 and geo["blocks"][2] <= 256
        assert all(p <= 256 for p in oracle["padded_shape"])               # register transforms, of 32 and of 256 points
    else:
        assert voxels <= mc.ITEMS_PER_TRIP and padded <= mc.ITEMS_PER_TRIP and window <= mc.ITEMS_PER_TRIP
        assert oracle["padded_shape"][-1] > 4096                           # the four-step transform
    # the answer
    assert oracle["status"] == mo.STATUS_OK and oracle["peak"] == case["offset"]
    assert f32["status"] == mo.STATUS_OK and f32["peak"] == case["offset"]
    r, eligible = oracle["r"], oracle["eligible"]
    far = eligible & _far_from(oracle["peak_window"], r.shape)
    assert far.any()
    margin = float(r[oracle["peak_window"]] - r[far].max())
    print(name, "peak r", r[oracle["peak_window"]], "margin", margin, "against", 100 * mc.GPU_R_TOLERANCE_LARGE[name])
    assert margin >= 100 * mc.GPU_R_TOLERANCE_LARGE[name]
    assert mc.GPU_R_TOLERANCE_LARGE[name] == 8 * mc.MEASURED_R_ERROR_LARGE[name]
    # the zeroing rule cannot flip between float32 and float64
    ratio = float((oracle["den"][eligible] / oracle["tol"]).min())
    print(name, "least den / tol over eligible shifts", ratio)
    assert ratio > 8.0
    # rint(N) has room: the restatement's N is within 1/16 of an integer at every shift, which leaves the GPU 8 times the
    # restatement's error before a count could change; and the counts are the exact ones
    off = float(np.abs(f32["n_raw"] - np.rint(f32["n_raw"])).max())
    print(name, "max |N - rint(N)| of the float32 restatement", off)
    assert f32["n_raw"].dtype == np.float32 and f32["n_raw"].shape == r.shape and off <= 1.0 / 16.0
    assert np.array_equal(f32["n"], oracle["n"]) and np.array_equal(f32["eligible"], eligible)
    # the validity the case intends is the validity the keyword arguments give, and the bright block is there
    assert np.array_equal(mo.validity(case["F"], None, None), case["vF"])
    assert np.array_equal(mo.validity(case["M"], case["kwargs"]["moving_mask"], None), case["vM"])
    assert np.nanmax(case["M"][~case["vM"]]) == mc.BRIGHT


@pytest.mark.parametrize("name", list(mc.LARGE_CASES))
def test_float32_restatement_matches_fft_float64(name):
    case, oracle, f32 = mc.case_with_oracle(name)
    err = float(np.abs(f32["r"].astype(np.float64) - oracle["r"])[oracle["eligible"]].max())
    print(name, "max |dr| over eligible shifts", err)
    assert err <= 2.0 * mc.MEASURED_R_ERROR_LARGE[name]
    assert list(mc.MEASURED_R_ERROR_LARGE) == list(mc.LARGE_CASES)


def test_swapped_large_case_is_the_reversed_window():
    """What the GPU test of the swapped crops relies on: r(moving, fixed)(s) = r(fixed, moving)(-s), the restatement's error on the
    swapped crops is within the figure of the case, and the peak then is the partial of a workgroup beyond the first 256."""
    name = "nan_520x520_shift_300"
    case, oracle, _ = mc.case_with_oracle(name)
    kw = dict(fixed_mask=case["kwargs"]["moving_mask"], max_shift=case["max_shift"])
    rev = tuple(slice(None, None, -1) for _ in oracle["r"].shape)
    fft = mo.fft_float64(case["M"], case["F"], **kw)
    assert np.array_equal(fft["n"], oracle["n"][rev]) and np.array_equal(fft["eligible"], oracle["eligible"][rev])
    assert fft["peak"] == [-k for k in case["offset"]] and fft["status"] == mo.STATUS_OK
    assert np.abs(fft["r"] - oracle["r"][rev])[fft["eligible"]].max() <= 1e-12
    f32 = mo.float32_chain(case["M"], case["F"], **kw)
    err = float(np.abs(f32["r"].astype(np.float64) - oracle["r"][rev])[fft["eligible"]].max())
    print(name, "swapped: max |dr| over eligible shifts", err)
    assert err <= 2.0 * mc.MEASURED_R_ERROR_LARGE[name] and np.array_equal(f32["n"], fft["n"])
    assert float(np.abs(f32["n_raw"] - np.rint(f32["n_raw"])).max()) <= 1.0 / 16.0
    flat = int(np.ravel_multi_index(fft["peak_window"], fft["r"].shape))
    assert flat == 150 * 601 + 311 and flat < mc.ITEMS_PER_TRIP and flat // 256 > 256


def _r_error(f32, brute):
    return float(np.abs(f32["r"].astype(np.float64) - brute["r"])[brute["eligible"]].max())


def test_value_edge_cases_meet_their_conditions():
    """What the GPU tests of the value edges rely on, by the oracle alone."""
    base, base_brute, _ = mc.case_with_oracle("nan_13x20")
    # infinities: six valid voxels fewer in each crop, the answer stays
    case, brute, f32 = mc.value_case("inf")
    for im, v in (("F", "vF"), ("M", "vM")):
        assert int(np.isinf(case[im]).sum()) == 6 and int(case[v].sum()) == int(base[v].sum()) - 6
        assert np.array_equal(mo.validity(case[im], case["kwargs"].get("moving_mask") if im == "M" else None, None), case[v])
    assert brute["status"] == mo.STATUS_OK and brute["peak"] == case["offset"] and not np.array_equal(brute["n"], base_brute["n"])
    assert np.array_equal(f32["n"], brute["n"]) and _r_error(f32, brute) <= 2.0 * mc.R_ERROR
    # camera offset: whole numbers around 30000 that float32 holds, r of the definition as without the offset
    case, brute, f32 = mc.value_case("camera")
    vals = case["F"][case["vF"]]
    assert np.array_equal(vals, np.rint(vals)) and 40.0 <= float(vals.max() - vals.min()) / 2 <= 60.0
    assert abs(float(vals.astype(np.float64).mean()) - mc.CAMERA_OFFSET) <= 10.0
    assert np.array_equal(case["F"].astype(np.float64) - mc.CAMERA_OFFSET, case["plain_F"].astype(np.float64), equal_nan=True)
    plain = mo.brute_force(case["plain_F"], case["plain_M"], **case["kwargs"])
    assert np.array_equal(plain["n"], brute["n"]) and np.abs(plain["r"] - brute["r"]).max() <= 1e-12
    assert brute["status"] == mo.STATUS_OK and brute["peak"] == case["offset"] and f32["peak"] == case["offset"]
    err = _r_error(f32, brute)
    uncentred = _r_error(mo.float32_chain(case["F"], case["M"], centre=False, **case["kwargs"]), brute)
    print("camera offset: max |dr| of the float32 restatement", err, "and without centring", uncentred)
    assert err <= 2.0 * mc.MEASURED_R_ERROR_CAMERA
    # the case bites: a chain that does not centre misses the bound of the GPU test, by far
    assert uncentred > 8 * mc.MEASURED_R_ERROR_CAMERA and uncentred >= 0.5 * mc.MEASURED_R_ERROR_CAMERA_UNCENTRED
    # valid_above at a value
    above, exact = 0.1, float(mc.THRESHOLD_VALUE)
    assert exact > above and np.float32(above) == mc.THRESHOLD_VALUE
    counts = {}
    for thr in (above, exact):
        case, brute, f32 = mc.value_case("threshold", valid_above=(thr, thr))
        at_value = [int((case[im] == mc.THRESHOLD_VALUE).sum()) for im in ("F", "M")]
        assert min(at_value) >= 30
        counts[thr] = [int(mo.validity(case[im], None, thr).sum()) for im in ("F", "M")]
        assert brute["status"] == mo.STATUS_OK and np.array_equal(f32["n"], brute["n"]) and _r_error(f32, brute) <= 2.0 * mc.R_ERROR
    assert [a - b for a, b in zip(counts[above], counts[exact])] == at_value
    # eligibility at equality
    case, brute, f32 = mc.value_case("eligibility", overlap_ratio=0.5)
    S = brute["shifts"]
    zz, xx = np.meshgrid(np.arange(-S[0], S[0] + 1), np.arange(-S[1], S[1] + 1), indexing="ij")
    assert np.array_equal(brute["n"], (8 - np.abs(zz)) * (16 - np.abs(xx))) and brute["n_max"] == 128
    planted = tuple(k + s for k, s in zip(case["offset"], S))
    assert brute["n"][planted] == 64 and brute["eligible"][planted] and brute["peak"] == case["offset"] == f32["peak"]
    other = mc.value_case("eligibility", overlap_ratio=0.51)[1]
    assert not other["eligible"][planted] and other["status"] == mo.STATUS_OK and other["peak"] != case["offset"]
    for res in (brute, other):      # each peak leads every other eligible shift by far more than the GPU tolerance
        rr = np.where(res["eligible"], res["r"], -np.inf)
        best = rr[res["peak_window"]]
        rr[res["peak_window"]] = -np.inf
        assert best - rr.max() >= 100 * mc.GPU_R_TOLERANCE


def test_oracle_status_order():
    """Too few valid voxels comes before a constant crop; exactly min_overlap valid voxels are enough."""
    rng = np.random.default_rng(2)
    a, b = rng.random((12, 14)).astype(np.float32), rng.random((12, 14)).astype(np.float32)
    three = np.full_like(b, np.nan)
    three[4, 3:6] = 7.0
    assert mo.brute_force(a, three)["status"] == mo.STATUS_TOO_FEW_VALID
    sixteen = np.full_like(b, np.nan)
    sixteen[2:6, 5:9] = b[2:6, 5:9]
    assert int(np.isfinite(sixteen).sum()) == 16 == 4 ** 2
    assert mo.brute_force(a, sixteen)["status"] == mo.STATUS_OK
    fifteen = sixteen.copy()
    fifteen[2, 5] = np.nan
    assert mo.brute_force(a, fifteen)["status"] == mo.STATUS_TOO_FEW_VALID


def test_oracle_statuses():
    rng = np.random.default_rng(0)
    a, b = rng.random((12, 14)).astype(np.float32), rng.random((12, 14)).astype(np.float32)
    assert mo.brute_force(a, np.full_like(b, np.nan))["status"] == mo.STATUS_TOO_FEW_VALID
    m = np.ones(a.shape, np.uint8)
    m[3:, :] = 0
    flat = b.copy()
    flat[:3, :] = 7.0
    assert mo.brute_force(a, flat, moving_mask=m)["status"] == mo.STATUS_CONSTANT_CROP
    left, right = np.zeros(a.shape, np.uint8), np.zeros(a.shape, np.uint8)
    left[:, :6], right[:, 8:] = 1, 1
    res = mo.brute_force(a, b, fixed_mask=right, moving_mask=left, overlap_ratio=1.0, max_shift=1)
    assert res["status"] == mo.STATUS_NO_ELIGIBLE_SHIFT and res["n_max"] == 0 and res["peak"] is None


def test_plan_header_under_sanitizers(tmp_path):
    """tests/native/masked_corr_plan_host_test.cpp: a stand-alone program of mvs_masked_corr_plan.h, built with the host compiler and
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "masked_corr_plan_host_test"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "masked_corr_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"

    n_ok = n_large = n_bad = 0
    for ln in lines:
        if not ln.startswith("P "):
            continue
        head, tail = ln[2:].split(":")
        ndim, *args = (int(v) for v in head.split())
        shape, ms = args[:3], args[3:]
        out = [int(v) for v in tail.split()]
        valid = ndim in (2, 3) and all(1 <= n < 2 ** 31 for n in shape) and (ndim == 3 or shape[0] == 1)
        if not valid:
            assert out == [1], ln
            n_bad += 1
            continue
        S = [n - 1 if (s < 0 or s > n - 1) else s for n, s in zip(shape, ms)]
        P = ops.padded_shape(shape, S)
        assert P == mo.padded_shape(shape, S)
        if int(np.prod([int(p) for p in P], dtype=object)) > _lib.MVS_MASKED_CORR_MAX_VOXELS:
            assert out == [2], ln
            n_large += 1
            continue
        W = [2 * s + 1 for s in S]
        blocks = lambda items: min(max((items + 255) // 256, 1), 1024)
        voxels, padded, window = int(np.prod(shape)), int(np.prod(P)), int(np.prod(W))
        assert out == [0, *S, *P, *W, voxels, padded, window, blocks(voxels), blocks(padded), blocks(window)], ln
        assert all(p & (p - 1) == 0 and (p >= n + s or n == 1) for p, n, s in zip(P, shape, S))
        assert window <= padded and voxels <= padded
        n_ok += 1
    assert n_ok >= 10 and n_large >= 4 and n_bad >= 4
    # the padded shapes of the test cases, as literals
    want = {"2 1 13 20 -1 -1 -1": [1, 32, 64], "3 6 9 11 -1 -1 -1": [16, 32, 32], "2 1 24 40 -1 5 7": [1, 32, 64], "2 1 1 17 -1 -1 -1": [1, 1, 64],
            "3 8 16 16 -1 -1 -1": [16, 32, 32], "2 1 5 31 -1 4 9": [1, 16, 64], "3 8 16 16 0 0 0": [8, 16, 16], "3 2 2 2 -1 -1 -1": [4, 4, 4]}
    got = {ln[2:].split(":")[0].strip(): [int(v) for v in ln.split(":")[1].split()][4:7] for ln in lines if ln.startswith("P ") and ln.split(":")[1].split()[0] == "0"}
    for key, P in want.items():
        assert got[key] == P, key
    # the large cases, as literals: S, P, W, voxels, padded, window, blocks of the three grids
    large = {"2 1 520 520 -1 300 300": [0, 300, 300, 1, 1024, 1024, 1, 601, 601, 270400, 1 << 20, 361201, 1024, 1024, 1024],
             "3 20 130 130 3 40 40": [3, 40, 40, 32, 256, 256, 7, 81, 81, 338000, 1 << 21, 45927, 1024, 1024, 180],
             "2 1 3 4100 -1 1 10": [0, 1, 10, 1, 4, 8192, 1, 3, 21, 12300, 1 << 15, 63, 49, 128, 1]}
    full = {ln[2:].split(":")[0].strip(): [int(v) for v in ln.split(":")[1].split()] for ln in lines if ln.startswith("P ")}
    for key, rest in large.items():
        assert full[key] == [0, *rest], key
    for c in mc.LARGE_CASES.values():
        shape3, shift3 = (1,) * (3 - len(c["shape"])) + c["shape"], (-1,) * (3 - len(c["shape"])) + c["max_shift"]
        assert " ".join(str(v) for v in (len(c["shape"]), *shape3, *shift3)) in large
    # window_to_padded of their first entry (the shift -S: P - S per axis) and of their last (+S)
    ends = {ln[2:].split(":")[0].strip(): [int(v) for v in ln.split(":")[1].split()] for ln in lines if ln.startswith("E ")}
    assert ends == {"1 520 520": [361201, 724 * 1024 + 724, 300 * 1024 + 300],
                    "20 130 130": [45927, (29 * 256 + 216) * 256 + 216, (3 * 256 + 40) * 256 + 40],
                    "1 3 4100": [63, 3 * 8192 + 8182, 1 * 8192 + 10]}

    alias = [[int(v) for v in ln[2:].replace(":", " ").split()] for ln in lines if ln.startswith("A ")]
    assert len(alias) >= 8
    for n, S, P, bad, half, bad_half in alias:
        assert P >= n + S and bad == 0, (n, S)                         # alias-free on the whole window
        if half < n + S and S > 0:
            assert bad_half > 0, (n, S)                                # and a shorter transform is not
    assert any(half < n + S and S > 0 for n, S, P, bad, half, bad_half in alias)
    w_line = next(ln for ln in lines if ln.startswith("W ")).split()
    assert w_line[1] == w_line[2] and w_line[3] == "0"
    assert next(ln for ln in lines if ln.startswith("G ")) == "G 1 1 1 2 1024"


def test_refusals_need_no_device():
    """Over the limit (NotImplementedError naming max_shift, and MVS_ERR_UNSUPPORTED from the C entry before it touches a device), a
    shape mismatch, a mask of another shape, overlap_ratio outside (0, 1]."""

    class Shaped:                      # a crop of which only the shape is ever looked at
        def __init__(self, shape):
            self.shape, self.dtype = shape, np.dtype(np.float32)

    with pytest.raises(NotImplementedError, match="max_shift"):
        registration.masked_correlation_registration(Shaped((400, 400, 400)), Shaped((400, 400, 400)))
    with pytest.raises(NotImplementedError, match="max_shift"):
        registration.masked_correlation_registration(Shaped((512, 512, 1024)), Shaped((512, 512, 1024)), max_shift=(0, 0, 1))
    assert ops.check_limit((512, 512, 1024), (0, 0, 0)) == (512, 512, 1024)
    assert ops.check_limit((400, 400, 400), (100, 100, 100)) == (512, 512, 512)
    a = np.zeros((8, 9), np.float32)
    with pytest.raises(ValueError, match="same shape"):
        registration.masked_correlation_registration(a, np.zeros((8, 10), np.float32))
    with pytest.raises(ValueError, match="fixed_mask"):
        registration.masked_correlation_registration(a, a, fixed_mask=np.ones((8, 10), np.uint8))
    with pytest.raises(ValueError, match="moving_mask"):
        registration.masked_correlation_registration(a, a, moving_mask=np.ones((9, 8), np.uint8))
    for ratio in (0.0, -0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match="overlap_ratio"):
            registration.masked_correlation_registration(a, a, overlap_ratio=ratio)
    with pytest.raises(ValueError, match="max_shift"):
        registration.masked_correlation_registration(a, a, max_shift=(1, 2, 3))
    with pytest.raises(ValueError, match="valid_above"):
        registration.masked_correlation_registration(a, a, valid_above=(1.0, 2.0, 3.0))
    assert _lib.MVS_MASKED_CORR_MAX_VOXELS == 2 ** 28

    lib = _lib.load()
    opts = _lib.mvs_masked_corr_opts_t()
    opts.ndim, opts.mem, opts.mask_mem, opts.overlap_ratio, opts.min_overlap = 3, _lib.MVS_MEM_HOST, _lib.MVS_MEM_HOST, 0.3, 64
    opts.max_shift[:] = [-1, -1, -1]
    res = _lib.mvs_masked_corr_result_t()
    tiny = np.zeros(8, np.float32)     # never read: the refusal comes first
    call = lambda shape: lib.mvs_masked_corr(0, tiny.ctypes.data, tiny.ctypes.data, None, None, _lib.i64x3(shape), C.byref(opts), C.byref(res), None, None)
    assert call((400, 400, 400)) == _lib.ERR_UNSUPPORTED
    assert b"max_shift" in lib.mvs_last_error(0)
    assert call((0, 4, 4)) == -1
    opts.overlap_ratio = 0.0
    assert call((2, 2, 2)) == -1
    opts.overlap_ratio, opts.ndim = 0.3, 2
    assert call((2, 2, 2)) == -1           # 2D crops have shape[0] == 1


def test_subpixel_offset():
    assert ops.subpixel_offset(1.0, 0.5, 0.5) == 0.0                                  # symmetric
    assert ops.subpixel_offset(1.0, 0.5, 0.75) == pytest.approx(0.5 * (0.5 - 0.75) / (0.5 - 2.0 + 0.75))
    assert ops.subpixel_offset(1.0, 0.5, 0.75) > 0 > ops.subpixel_offset(1.0, 0.75, 0.5)      # towards the larger neighbour
    # an exact parabola r = 1 - (x - 0.3)^2 sampled at -1, 0, 1
    f = lambda x: 1.0 - (x - 0.3) ** 2
    assert ops.subpixel_offset(f(0), f(-1), f(1)) == pytest.approx(0.3, abs=1e-12)
    assert ops.subpixel_offset(0.7, 0.7, 0.7) == 0.0                                  # flat: no curvature
    assert ops.subpixel_offset(0.5, 0.6, 0.6) == 0.0                                  # positive curvature
    assert ops.subpixel_offset(1.0, 0.5, 0.75, left_ok=False) == 0.0                  # an ineligible neighbour
    assert ops.subpixel_offset(1.0, 0.5, 0.75, right_ok=False) == 0.0
    assert ops.subpixel_offset(1.0, np.nan, 0.75) == 0.0                              # outside the window
    assert ops.subpixel_offset(1.0, 0.0, 1.0) == 0.5                                  # the clamp (the vertex lies at 0.5 exactly)
    assert ops.subpixel_offset(1.0, 1.0 + 1e-9, 0.0) == -0.5                          # ... and beyond it
    assert ops.subpixel_offset(0.9, 0.1, 0.9 - 1e-12) == pytest.approx(0.5, abs=1e-9)
    # the oracle's helper agrees on a volume
    r = np.array([[0.1, 0.2, 0.1], [0.3, 0.9, 0.5], [0.2, 0.4, 0.1]])
    delta, curv = mo.subpixel(r, np.ones(r.shape, bool), (1, 1))
    assert delta == [ops.subpixel_offset(0.9, 0.2, 0.4), ops.subpixel_offset(0.9, 0.3, 0.5)] and all(c < 0 for c in curv)
    el = np.ones(r.shape, bool)
    el[1, 2] = False
    assert mo.subpixel(r, el, (1, 1))[0][1] == 0.0 and mo.subpixel(r, el, (0, 1))[0][0] == 0.0
