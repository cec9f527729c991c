"""CPU: the host side of ``masks.feather``: its scipy oracle against the definition, the argument for 252, the integer scheme of the
kernel restated in numpy against the oracle, width parsing and the refusals that need no device, and
csrc/mvs_mask_feather_plan.h compiled for the host under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _mask_ops, masks
from multiview_stitcher_amd import spatial_image_utils as si
from tests import mask_feather_cases as fc
from tests import mask_feather_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ("thin_stack", "one_plane_w32", "long_rows", "plane_40x67", "tiny_w32")


@pytest.mark.parametrize("shape,width", [((4, 5, 6), (2, 3, 4)), ((7, 9), (3, 2)), ((3, 4, 5), (32, 32, 32)), ((1, 6, 7), (1, 5, 2)), ((5, 6), 0)])
def test_oracle_is_the_definition_on_tiny_masks(shape, width):
    mask = fc.blob_mask(shape, seed=3, sigma=1.0)
    assert 0 < mask.sum() < mask.size
    want = fo.brute_force_distance(mask, width)
    assert np.abs(fo.capped_distance(mask, width) - want).max() <= 1e-12
    assert np.array_equal(fo.feather(mask, width), np.rint(fo.ramp(want)).astype(np.uint8))
    assert np.all(fo.feather(mask, width)[mask == 0] == 0)


def test_252_is_an_integer_at_the_rational_points():
    """cos(pi t) is rational only at t = 0, 1/3, 1/2, 2/3, 1 (Niven); the ramp there is 0, 1/4, 1/2, 3/4, 1 and 252 of each an
    integer, so an exact tie never reaches the rounding -- with 255 the value at t = 1/2 would be 127.5."""
    for t, part in ((0.0, 0), (1.0 / 3.0, 63), (0.5, 126), (2.0 / 3.0, 189), (1.0, 252)):
        assert abs(fo.ramp(t) - part) < 1e-12 and 4 * part % 252 == 0
        assert int(np.rint(fo.ramp(t))) == part
    assert 255 * 0.5 == 127.5 and masks.FULL_WEIGHT == fo.FULL_WEIGHT == _lib.MVS_FEATHER_FULL_WEIGHT == 252


def test_masks_without_zero_and_without_nonzero():
    assert np.all(fo.feather(np.ones((3, 4, 5), np.uint8), (2, 2, 2)) == 252)
    assert np.all(fo.feather(np.full((4, 5), 7, np.uint8), 3) == 252)          # nonzero means "use"
    assert np.all(fo.feather(np.zeros((3, 4, 5), np.uint8), (2, 2, 2)) == 0)
    hard = fo.feather(fc.blob_mask((9, 11)), 0)                                 # no feather: 0 or 252
    assert np.array_equal(hard, fc.blob_mask((9, 11)) * np.uint8(252))


def integer_scheme(mask, width):
    """The kernel's arithmetic in numpy: D = prod w^2, P_k = D / w_k^2, N = min(D, min_q sum_k d_k^2 P_k) by separable min-plus
    passes x, y, z capped at D after each, then sqrt(N / D) and the cosine in float64."""
    mask = np.asarray(mask) != 0
    w = fo.widths_of(width, mask.ndim)
    D = int(np.prod([k * k for k in w]))
    assert D <= 2 ** 30
    N = np.where(mask, D, 0).astype(np.int64)
    for axis in range(mask.ndim - 1, -1, -1):
        P, n = D // (w[axis] * w[axis]), mask.shape[axis]
        prev, best = N, N.copy()
        for j in range(1, min(w[axis], n - 1) + 1):
            lo = [slice(None)] * mask.ndim
            hi = [slice(None)] * mask.ndim
            lo[axis], hi[axis] = slice(0, n - j), slice(j, n)
            lo, hi = tuple(lo), tuple(hi)
            best[lo] = np.minimum(best[lo], prev[hi] + j * j * P)
            best[hi] = np.minimum(best[hi], prev[lo] + j * j * P)
        N = np.minimum(best, D)
        assert N.max() + w[axis] * w[axis] * P < 2 ** 32
    return N, np.rint(fo.ramp(np.sqrt(N / D))).astype(np.uint8)


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_integer_scheme_equals_the_oracle(name):
    shape, width = fc.CASES[name]
    mask = fc.blob_mask(shape)
    want_f = fo.feather_float(mask, width)
    assert fo.half_integer_distance(want_f) > (1e-6 if name in FIVE else 1e-9)      # no value sits on a rounding edge
    N, got = integer_scheme(mask, width)
    assert np.array_equal(got, fo.feather(mask, width))
    t = fo.capped_distance(mask, width)
    D = int(np.prod([k * k for k in fo.widths_of(width, mask.ndim)]))
    assert np.abs(N / D - t * t).max() <= 1e-12                                      # N is D t^2 capped, exactly an integer
    assert 0 < (got == 0).sum() < got.size and ((got > 0) & (got < 252)).any()


def test_width_parsing_and_refusals():
    assert _mask_ops.check_feather_width(0, 3) == [1, 1, 1]
    assert _mask_ops.check_feather_width(5, 2) == [5, 5]
    assert _mask_ops.check_feather_width((1, 32), 2) == [1, 32]
    for bad in (33, -1, (0, 3), (2, 40), (1, 2, 3)):
        with pytest.raises(ValueError, match="32|one feather width"):
            _mask_ops.check_feather_width(bad, 2)
    with pytest.raises(TypeError):
        _mask_ops.check_feather_width((1.5, 2), 2)
    mask = np.ones((4, 5), np.uint8)
    with pytest.raises(ValueError, match="32"):
        masks.feather(mask, 33)
    with pytest.raises(ValueError, match="32"):
        masks.feather(mask, {"x": 3})                # a dict names every dim: y would be 0
    with pytest.raises(ValueError, match="32"):
        masks.feather(mask, (0, 3))
    with pytest.raises(TypeError, match="uint8"):
        masks.feather(mask.astype(np.uint16), 3)
    with pytest.raises(ValueError, match="2-D or 3-D"):
        masks.feather(np.ones(5, np.uint8), 3)
    assert list(inspect.signature(masks.feather).parameters) == ["mask", "width", "device", "keep_on_device"]
    assert inspect.signature(masks.feather).parameters["keep_on_device"].default is False


@pytest.mark.parametrize("dim", ["t", "c"])
def test_sims_with_t_or_c_dims_are_refused_by_name(dim):
    sim = si.to_spatial_image(np.ones((1, 4, 5), np.uint8), dims=[dim, "y", "x"], scale={"y": 1.0, "x": 1.0}, translation={"y": 0.0, "x": 0.0})
    with pytest.raises(ValueError, match=f"'{dim}' dim"):
        masks.feather(sim, 3)


def test_entry_point_checks_its_limits_before_it_needs_a_device():
    lib = _lib.load()
    view = _lib.mvs_view_t()
    data = np.ones((1, 4, 16), np.uint8)
    view.data, view.dtype, view.mem = data.ctypes.data, _lib.MVS_U8, _lib.MVS_MEM_HOST
    view.shape[:] = data.shape
    view.stride[:] = [64, 16, 1]
    out = np.zeros(data.shape, np.uint8)
    call = lambda ndim, w: lib.mvs_mask_feather(0, C.byref(view), ndim, (C.c_int32 * 3)(*w), C.c_void_p(out.ctypes.data), _lib.MVS_MEM_HOST)
    assert call(3, (1, 1, 33)) == _lib.ERR_UNSUPPORTED
    assert call(3, (1, 0, 4)) not in (0, _lib.ERR_UNSUPPORTED)
    assert call(4, (1, 1, 1)) not in (0, _lib.ERR_UNSUPPORTED)
    assert _lib.MVS_FEATHER_MAX_WIDTH == 32


def test_plan_header_under_sanitizers(tmp_path):
    """tests/native/mask_feather_plan_host_test.cpp: a stand-alone program of mvs_mask_feather_plan.h, built with the host compiler
    and -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "mask_feather_plan_host_test"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "mask_feather_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    scales = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("S ")]
    assert len(scales) == 6 ** 3
    for wz, wy, wx, D, pz, py, px, worst in scales:
        assert D == (wz * wy * wx) ** 2 <= 2 ** 30
        assert (pz, py, px) == (D // wz ** 2, D // wy ** 2, D // wx ** 2)
        assert worst == 2 * D < 2 ** 32                    # a capped value plus the largest term of a pass fits uint32
    slabs = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("L ")]
    assert len(slabs) == 7 * 4 * 5 + 2 and all(row[-1] == 1 for row in slabs)
    by_key = {tuple(row[:5]): row for row in slabs if row[5] == 256 << 20}
    assert by_key[(256, 256, 256, 32, 0)][6:8] == [256, 1]                 # 256^3 with a halo of 32: one slab (128 MiB of plane sets)
    assert by_key[(1000, 2048, 2048, 32, 0)][6:8] == [1, 1000]             # the budget holds 8 planes, the halo alone is 64: slabs of one plane
    assert by_key[(12, 20, 37, 3, 5)][6:8] == [5, 3]
    small = [row for row in slabs if row[5] == 1 << 20][0]
    assert small[6:8] == [1, 64]                                            # 13 planes fit, the halo is 16
    assert [int(v) for v in next(ln for ln in lines if ln.startswith("P ")).split()[1:]] == [0, 0, 1, 1]
