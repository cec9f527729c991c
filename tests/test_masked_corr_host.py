"""CPU: the masked correlation (registration.masked_correlation_registration) without a device: conditions on the test cases that
the oracle alone checks, the float32 restatement of the device chain against the float64 brute force (it sizes the GPU tolerances),
csrc/mvs_masked_corr_plan.h compiled for the host under the address and undefined-behaviour sanitizers, the refusals that need no
device and the sub-pixel parabola."""
import ctypes as C
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
