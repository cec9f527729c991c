"""CPU tests of the shading correction: the radix select of csrc/mvs_stack_select.h compiled for the host
(tests/native/stack_select_host_test.cpp), the sort-based oracle against numpy's own quantiles, the host algebra of
intensity.shading_from_planes / shading_coefficients against hand values and against the oracle's restatement, and the recovery
of a planted profile from the oracle's planes.

Recovery errors max |F / F0 - 1| measured with the oracle's planes: 0.0156 (24 tiles of 24 x 64 x 64) and 0.0118 (144 tiles of
96 x 96), float32 and uint16 alike; over four seeds 0.015 .. 0.022 and 0.006 .. 0.025 (tests/shading_helpers.py).
The cap of 0.05 is the condition the end-to-end bounds of tests/test_shading_gpu.py are derived from."""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from multiview_stitcher_amd import _shading_ops, intensity
from tests import shading_oracle as so
from tests.shading_helpers import CASES, RECOVERY_CAP, oracle_planes, planted_case, recovery_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the selection on the host ---------------------------------------------------------------------------------------------------
def test_radix_select_keys_ranks_and_strips_on_the_host(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "stack_select_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "stack_select_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    stacks = {ln.split()[1]: [int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("S ")}
    assert sorted(stacks) == ["f32", "u16", "u8"]
    for name, (n, wrong) in stacks.items():
        assert n >= 70 and wrong == 0, f"{name}: {wrong} of {n} stacks selected the wrong sample"
    assert next(ln for ln in lines if ln.startswith("K ")).split()[1] == "0"
    assert next(ln for ln in lines if ln.startswith("R ")).split()[1] == "0"
    widths, wrong = (int(v) for v in next(ln for ln in lines if ln.startswith("P ")).split()[1:])
    assert widths == 3300 and wrong == 0


def test_rank_of_is_numpys_lower_rank():
    for n in (1, 2, 3, 255, 256, 257, 70000):
        for q in (0, 0.02, 0.5, 0.73, 1):
            assert _shading_ops.rank_of(n, q) == int(np.floor((n - 1) * q))
    assert np.array_equal(_shading_ops.rank_of(np.array([0, 1, 5]), 0.5), [0, 0, 2])


# ---- the oracle against numpy -------------------------------------------------------------------------------------------------------
Q5 = (0, 0.02, 0.5, 0.73, 1)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_oracle_planes_are_numpys_lower_quantiles(dtype):
    rng = np.random.default_rng(3)
    if dtype == np.float32:
        tiles = [(rng.standard_normal((z, 5, 9)) * 3).astype(np.float32) for z in (3, 7, 1)]
        for t in tiles:
            t[rng.random(t.shape) < 0.2] = np.nan
        tiles[0][:, 0, 0], tiles[1][:, 0, 0], tiles[2][:, 0, 0] = np.nan, np.nan, np.nan          # a pixel without samples
    else:
        tiles = [rng.integers(0, np.iinfo(dtype).max + 1, size=(z, 5, 9)).astype(dtype) for z in (3, 7, 1)]
    planes, counts = so.stack_quantiles(tiles, Q5)
    stack = so.stack_of(tiles)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                            # (numpy warns about the all-NaN pixel)
        want = np.stack([(np.nanquantile if dtype == np.float32 else np.quantile)(stack, q, axis=0, method="lower") for q in Q5])
    assert np.array_equal(planes, want.astype(np.float32), equal_nan=True)
    assert np.array_equal(counts, (~np.isnan(stack.astype(np.float64))).sum(axis=0))
    if dtype == np.float32:
        assert counts[0, 0] == 0 and np.isnan(planes[:, 0, 0]).all()


# ---- the host algebra: hand values ---------------------------------------------------------------------------------------------------
def test_shading_coefficients_by_hand():
    shading = {"flatfield": np.float32([[0.5, 1.0], [2.0, 4.0]]), "darkfield": np.float32([[1.0, 2.0], [3.0, 4.0]]), "offset": 2.5}
    c = intensity.shading_coefficients(shading)
    assert c.shape == (2, 2, 2) and c.dtype == np.float32
    assert np.array_equal(c[..., 0], np.float32([[2.0, 1.0], [0.5, 0.25]]))
    assert np.array_equal(c[..., 1], np.float32([[0.5, 0.5], [1.0, 1.5]]))           # 2.5 - D / F
    x = np.float32([[3.0, 5.0], [7.0, 9.0]])
    assert np.array_equal(so.apply(x, c), (x - shading["darkfield"]) / shading["flatfield"] + np.float32(2.5))


def test_shading_from_planes_raw_plane_by_hand():
    """No smoothing: F = R / mean(R) with masked pixels at the mean of the others, then the clamp."""
    plane = np.array([[2.0, 4.0, 6.0], [8.0, np.nan, 0.1]])
    counts = np.array([[9, 9, 9], [9, 9, 9]])
    counts[0, 0] = 3                                                              # too few samples: left out, filled with the mean
    got = intensity.shading_from_planes(plane[None], counts, degree=None, min_samples=8, min_flat=0.1)
    valid_mean = (4.0 + 6.0 + 8.0 + 0.1) / 4                                      # of the pixels with enough samples and a finite R
    filled = np.array([[valid_mean, 4.0, 6.0], [8.0, valid_mean, 0.1]])
    want = np.maximum(filled / filled.mean(), 0.1)
    assert want[1, 2] == 0.1 and want[0, 0] == want[1, 1]                         # the clamp holds, the masked pixels are filled
    np.testing.assert_allclose(got["flatfield"], want.astype(np.float32), rtol=1e-6)
    assert got["offset"] == 0.0 and not got["darkfield"].any()
    dark = intensity.shading_from_planes(plane[None], counts, darkfield=1.5, degree=None)
    assert dark["offset"] == 1.5 and np.all(dark["darkfield"] == 1.5)
    filled_d = np.where(np.isnan(plane) | (counts < 8), valid_mean, plane) - 1.5
    np.testing.assert_allclose(dark["flatfield"], np.maximum(filled_d / filled_d.mean(), 0.1).astype(np.float32), rtol=1e-6)


def test_polynomial_fit_reproduces_a_polynomial_and_ignores_masked_pixels():
    h, w = 20, 31
    y, x = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    poly = 2.0 + 0.3 * y - 0.2 * x * x + 0.1 * x * y ** 3                         # total degree 4
    plane = poly.copy()
    counts = np.full((h, w), 20)
    plane[3, 4], counts[7, 8] = np.inf, 1                                         # a non-finite sample and a starved pixel ...
    plane[7, 8] = 1e6                                                             # ... with a value that would wreck the fit
    got = intensity.shading_from_planes(plane[None], counts)
    np.testing.assert_allclose(got["flatfield"], poly / poly.mean(), rtol=2e-6)
    two = intensity.shading_from_planes(np.stack([0.25 * poly, plane]), counts, darkfield="quantile")
    np.testing.assert_allclose(two["darkfield"], 0.25 * poly, rtol=2e-6)
    np.testing.assert_allclose(two["flatfield"], poly / poly.mean(), rtol=2e-6)
    assert abs(two["offset"] - 0.25 * poly.mean()) < 1e-6
    with pytest.raises(ValueError):
        intensity.shading_from_planes(plane[None], np.zeros((h, w), int))


@pytest.mark.parametrize("kw", [dict(degree=4), dict(degree=2), dict(degree=None, sigma=3.0), dict(degree=None)])
def test_shading_from_planes_matches_the_restatement(kw):
    """The package accumulates normal equations in row blocks, the oracle solves the dense least squares: float64 both, so they
    agree far below the float32 the result is stored in (1e-6 relative allows for the normal equations' squared condition)."""
    planes, counts = oracle_planes("tiles2d", "f32")
    counts = counts.copy()
    counts[:3, :5] = 2
    case = planted_case("tiles2d", "f32")
    got = intensity.shading_from_planes(planes, counts, darkfield=case["dark"], **kw)
    want = so.shading_from_planes(planes, counts, darkfield=case["dark"], **kw)
    np.testing.assert_allclose(got["flatfield"], want["flatfield"], rtol=1e-6)
    assert np.array_equal(got["darkfield"], want["darkfield"]) and got["offset"] == want["offset"]
    assert np.array_equal(intensity.shading_coefficients(want), so.coefficients(want))


# ---- recovery of a planted profile ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["f32", "u16"])
@pytest.mark.parametrize("name", list(CASES))
def test_a_planted_profile_is_recovered_from_the_oracle_planes(name, dtype_name):
    case = planted_case(name, dtype_name)
    assert 0.40 < np.abs(case["flat"] - 1).max() < 0.46                            # "up to 43 % from 1"
    planes, counts = oracle_planes(name, dtype_name)
    shading = intensity.shading_from_planes(planes, counts, darkfield=case["dark"])
    err = recovery_error(shading, case)
    print(f"{name} {dtype_name}: max |F / F0 - 1| = {err:.4f}")
    assert err <= RECOVERY_CAP
    assert abs(shading["offset"] - case["dark"].mean()) <= 1e-6 * case["scale"]
