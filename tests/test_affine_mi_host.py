"""CPU: the host side of affine_registration(metric="mattes") -- the per-sample header (csrc/mvs_affine_mi_dev.h) compiled for
the host equals the float32 mode of the numpy restatement (tests/affine_mi_oracle.py) bit for bit, the restatement's analytic
gradient equals central differences of its metric, its loop recovers a pose across an intensity relation that the
squared-residual loop cannot, the loop of _affine_reg.py walks the restatement's iterations, and the public interface."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import affine_mi_oracle as mo
from tests import affine_reg_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(tokens):
    return np.array([int(t, 16) for t in tokens], dtype=np.uint32).view(np.float32)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


# ---- 1. the header on the host ------------------------------------------------------------------------------------------------
def test_header_equals_the_oracle_float32_mode_bit_for_bit(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "affine_mi_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "affine_mi_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"

    # the window functions on t = -2.5 .. 2.5 in steps of 1 / 1024
    T = [ln.split()[1:] for ln in lines if ln.startswith("T ")]
    assert len(T) == 5121
    t = _f32([row[0] for row in T])
    np.testing.assert_array_equal(t, (np.arange(5121) - 2560) / 1024.0)
    w = mo.beta3(t)
    assert w.dtype == np.float32 and _same_bits(_f32([row[1] for row in T]), w)
    assert _same_bits(_f32([row[2] for row in T]), mo.beta3_prime(t))
    np.testing.assert_array_equal(np.array([int(row[3]) for row in T]), mo.quantise(w))
    assert w[2560] == np.float32(2.0 / 3.0) and w[0] == 0 and w[-1] == 0 and mo.quantise(w).max() == 699051

    # bins, weights and the gradient weight of swept values
    R = {int(row[1]): _f32(row[2:]) for row in (ln.split() for ln in lines if ln.startswith("R "))}
    assert sorted(R) == [8, 32, 64]
    for B in (8, 32, 64):
        V = [ln.split()[2:] for ln in lines if ln.startswith(f"V {B} ")]
        assert len(V) == 10000
        lo, f_scale, m_scale = R[B]
        hi = np.float32(3.7)
        assert f_scale == np.float32((B - 1) / (float(hi) - float(lo))) and m_scale == np.float32((B - 4) / (float(hi) - float(lo)))
        v = _f32([row[0] for row in V])
        assert v[0] == lo and v[1] == hi and v.min() == lo and v.max() == hi
        a = np.array([int(row[1]) for row in V])
        np.testing.assert_array_equal(a, mo.fixed_bin(v, lo, f_scale, B))
        assert a[0] == 0 and a[1] == B - 1 and set(a) == set(range(B))
        u = mo.moving_coord(v, lo, m_scale, B)
        assert _same_bits(_f32([row[2] for row in V]), u)
        assert u[0] == 1.5 and u[1] == B - 2.5
        b0, args = mo.window(u)
        np.testing.assert_array_equal(np.array([int(row[3]) for row in V]), b0)
        assert b0.min() == 0 and b0.max() == B - 4                   # all four taps inside 0..B-1
        q = np.array([[int(x) for x in row[4:8]] for row in V])
        np.testing.assert_array_equal(q, np.stack([mo.quantise(mo.beta3(args[k])) for k in range(4)], axis=1))
        assert np.abs(q.sum(axis=1) - 2 ** 20).max() <= 2
        row_values = ((np.arange(B) * 37 % 11).astype(np.float32) - np.float32(5.0)) * np.float32(0.25)
        wg = mo.beta3_prime(args[0]) * row_values[b0]
        for k in range(1, 4):
            wg = wg + mo.beta3_prime(args[k]) * row_values[b0 + k]
        assert wg.dtype == np.float32 and _same_bits(_f32([row[8] for row in V]), wg)


# ---- 2. gradient against finite differences -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,model", [((64, 64), "rigid"), ((24, 32, 32), "affine")], ids=["2d-rigid", "3d-affine"])
def test_oracle_gradient_equals_central_differences(shape, model):
    """float64 mode, step 1e-5, 1e-3 relative per component (a 2D prototype measured 4e-5; the bound leaves room for the 3D case
    and the larger parameter count).  The metric is differentiable only while the set of valid samples stays the same and no
    sample sits on a knot of the interpolant: the pose is off the voxel grid, and the fixed crop is NaN wherever the pose puts a
    sample within half a voxel of the moving crop's border, so no perturbed pose changes the set.  Measured: 3.4e-4 (2D),
    2.6e-4 (3D), the rest being samples that cross a knot of the linear interpolant within the step."""
    B, h = 32, 1e-5
    nd = len(shape)
    F, M, _, _ = mo.make_pair(shape, 0, model)
    A, t = ao.true_pose(model, nd, 5, t0=(0.37, -0.21, 0.43)[3 - nd:])
    A = np.eye(nd) + 0.5 * (A - np.eye(nd))
    p, _ = ao.coordinates(shape, A, t)
    inside = np.ones(shape, dtype=bool)
    for k in range(nd):
        inside &= (p[k] >= 0.5) & (p[k] <= shape[k] - 1.5)
    assert 0.7 < inside.mean() < 0.95
    F = np.where(inside, F, np.float32(np.nan))
    rng = mo.ranges(F, M, B)
    mi, table, n, _ = mo.metric(F, M, A, t, B, rng, np.float64)
    assert n == inside.sum()
    g = ao.jacobian(model, A).T @ mo.gradient(F, M, A, t, B, rng, table, np.float64)
    nq = ao.n_params(model, nd)
    fd = np.zeros(nq)
    for k in range(nq):
        e = np.zeros(nq)
        e[k] = h
        plus = mo.metric(F, M, *ao.update(model, A, t, e), B, rng, np.float64)
        minus = mo.metric(F, M, *ao.update(model, A, t, -e), B, rng, np.float64)
        assert plus[2] == n and minus[2] == n
        fd[k] = (plus[0] - minus[0]) / (2 * h)
    rel = np.abs(g - fd) / np.abs(fd)
    print(f"{shape} {model}: MI {mi:.4f}, n {n}, |gradient - central difference| / |central difference|: max {rel.max():.2e}")
    assert np.all(rel <= 1e-3), rel


# ---- 3. the loop ----------------------------------------------------------------------------------------------------------
def needs_mi_pair():
    """64 x 64 smooth noise (Gaussian sigma 3), rotation 0.06 rad, shift (1.7, -2.3) px, moving remapped by |2 v - 2 median(v)|."""
    a = 0.06
    A0 = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return mo.make_pair((64, 64), 1, "rigid", sigma=3.0, A0=A0, t0=np.array([1.7, -2.3]))


def test_oracle_loop_recovers_a_pose_the_squared_residual_loop_cannot():
    """Start at identity.  The MI loop ends within 0.05 px of the truth (measured 0.006); the squared-residual loop ends more
    than 1 px away (measured 11.7, with a gain of 0.26): the case needs the metric."""
    F, M, A0, t0 = needs_mi_pair()
    out = mo.register(F, M, "rigid")
    err = ao.corner_displacement(out["A"], out["t"], A0, t0, F.shape)
    ssd = ao.register(F, M, "rigid")
    err_ssd = ao.corner_displacement(ssd["A"], ssd["t"], A0, t0, F.shape)
    print(f"MI loop: {err:.4f} px after {len(out['history'])} iterations, quality {out['quality']:.3f}; "
          f"squared-residual loop: {err_ssd:.2f} px, gain {ssd['history'][-1]['gain']:.2f}")
    assert err <= 0.05
    assert err_ssd > 1.0
    assert 0.0 < out["quality"] <= 1.0


@pytest.mark.parametrize("shape,model", [((41, 48), "rigid"), ((21, 37, 44), "affine")], ids=["2d-rigid", "3d-affine"])
def test_host_loop_on_the_oracle_metric_equals_the_oracle_loop(shape, model):
    """_affine_reg.optimise_mi driven by the restatement's histogram, gradient and preconditioner (no device) walks the
    restatement's iterations: the direction, its scaling, the backtracking, the level conversion on odd lengths and the stop
    rules agree.  _affine_reg.mutual_information equals the restatement's on a histogram with empty bins."""
    from multiview_stitcher_amd import _affine_reg as ar

    F, M, A0, t0 = mo.make_pair(shape, 2, model, t0=(0.9, -0.7, 0.5)[3 - len(shape):])
    want = mo.register(F, M, model, max_iterations=(8, 5))
    bins, B = (2, 1), 32
    crops = [(ao.bin_mean(F, b), ao.bin_mean(M, b)) for b in bins]
    rngs = [mo.ranges(f, m, B) for f, m in crops]
    for (f, m), rng in zip(crops, rngs):
        lo_hi = mo.finite_range(f) + mo.finite_range(m)
        assert [float(v) for v in ar.bin_ranges(*lo_hi, B)] == [float(v) for v in rng]

    def metric(li, A, tb):
        hist, n = mo.joint_hist(crops[li][0], crops[li][1], A, tb, B, rngs[li])
        mi, table, _ = ar.mutual_information(hist)
        return mi, table.astype(np.float32), n

    gradient = lambda li, A, tb, table: mo.gradient(crops[li][0], crops[li][1], A, tb, B, rngs[li], table)   # noqa: E731
    precond = lambda li, A, tb: ao.normal_equations(crops[li][0], crops[li][1], A, tb, 1.0, 0.0, np.float32)[0]   # noqa: E731
    nd = len(shape)
    A, t, history = ar.optimise_mi(metric, gradient, precond, bins, shape, model, np.eye(nd), np.zeros(nd), (8, 5), 1e-3)
    assert [(h["level"], h["alpha"], h["n"]) for h in history] == [(h["level"], h["alpha"], h["n"]) for h in want["history"]]
    assert {h["level"] for h in history} == {0, 1} and min(h["alpha"] for h in history) < 1.0
    np.testing.assert_allclose([h["mi"] for h in history], [h["mi"] for h in want["history"]], rtol=1e-12)
    np.testing.assert_allclose(A, want["A"], atol=1e-9)
    np.testing.assert_allclose(t, want["t"], atol=1e-9)

    hist, _ = mo.joint_hist(F, M, A, t, B, mo.ranges(F, M, B))
    assert (hist == 0).any()
    got, ref = ar.mutual_information(hist), mo.mutual_information(hist)
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-12)
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-12)
    assert 0.0 < got[2] <= 1.0

    # refusals of the loop: too few samples, a preconditioner that is not positive definite, a constant crop
    P = nd * (nd + 1)
    few = lambda *a: (0.5, np.zeros((B, B), np.float32), 4 * ar.n_model_params(model, nd) - 1)   # noqa: E731
    with pytest.raises(ar.Refused):
        ar.optimise_mi(few, gradient, precond, (1,), shape, model, np.eye(nd), np.zeros(nd), (5,), 1e-3)
    ok = lambda *a: (0.5, np.zeros((B, B), np.float32), 10000)   # noqa: E731
    with pytest.raises(ar.Refused):
        ar.optimise_mi(ok, lambda *a: np.ones(P), lambda *a: np.zeros((P, P)), (1,), shape, model, np.eye(nd), np.zeros(nd), (5,), 1e-3)
    with pytest.raises(ar.Refused):
        ar.bin_ranges(0.25, 0.25, 0.0, 1.0, B)
    with pytest.raises(ar.Refused):
        ar.bin_ranges(0.0, 1.0, np.nan, np.nan, B)


# ---- 4. public interface -----------------------------------------------------------------------------------------------------
def test_public_interface_has_metric_and_n_bins():
    from multiview_stitcher_amd import _affine_reg, _lib, registration

    for fn in (registration.affine_registration, _affine_reg.affine_registration):
        params = inspect.signature(fn).parameters
        assert params["metric"].default == "ssd" and params["n_bins"].default == 32
    for name in ("mvs_affine_joint_hist", "mvs_affine_mi_gradient", "mvs_finite_range"):
        assert name in _lib.SIGNATURES


def test_bad_metric_and_bad_n_bins_raise_before_any_library_call(monkeypatch):
    from multiview_stitcher_amd import _lib, registration

    def no_library(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "init", no_library)
    monkeypatch.setattr(_lib, "load", no_library)
    a = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError, match="metric"):
        registration.affine_registration(a, a, metric="mutual_information")
    for bad in (7, 65, 0, -32, 32.0, None):
        with pytest.raises(ValueError, match="n_bins"):
            registration.affine_registration(a, a, metric="mattes", n_bins=bad)
    with pytest.raises(ValueError, match="n_bins"):
        registration.affine_registration(a, a, n_bins=4)


def test_bad_arguments_return_error_codes():
    """ndim outside {2, 3}, n_bins outside 8..64, NULL pointers and non-positive shapes are refused before anything touches a
    device."""
    from multiview_stitcher_amd import _lib

    lib = _lib.load()
    a = np.zeros((4, 5, 6), np.float32)
    A, t = np.eye(3), np.zeros(3)
    hist, n = np.zeros(64 * 64, np.int64), C.c_int64()
    table, out = np.zeros(64 * 64, np.float32), np.zeros(_lib.MVS_AFFINE_MI_GRAD_LEN)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))       # noqa: E731
    ip = hist.ctypes.data_as(C.POINTER(C.c_int64))
    fp = table.ctypes.data_as(C.POINTER(C.c_float))

    def both(f, m, nd, shp, B):
        return (lib.mvs_affine_joint_hist(0, f, m, 0, nd, _lib.i64x3(shp), dp(A), dp(t), B, 0.0, 1.0, 0.0, 1.0, ip, C.byref(n)),
                lib.mvs_affine_mi_gradient(0, f, m, 0, nd, _lib.i64x3(shp), dp(A), dp(t), B, 0.0, 1.0, 0.0, 1.0, fp, dp(out)))

    p = a.ctypes.data
    assert both(p, p, 4, a.shape, 32) == (-1, -1)
    assert both(p, p, 1, a.shape, 32) == (-1, -1)
    assert both(None, p, 3, a.shape, 32) == (-1, -1)
    assert both(p, None, 3, a.shape, 32) == (-1, -1)
    assert both(p, p, 3, (4, 0, 6), 32) == (-1, -1)
    assert both(p, p, 2, (4, 5, 6), 32) == (-1, -1)
    assert both(p, p, 3, a.shape, 7) == (-1, -1)
    assert both(p, p, 3, a.shape, 65) == (-1, -1)
    assert lib.mvs_affine_joint_hist(0, p, p, 0, 3, _lib.i64x3(a.shape), dp(A), dp(t), 32, 0.0, 1.0, 0.0, 1.0, None, C.byref(n)) == -1
    assert lib.mvs_affine_mi_gradient(0, p, p, 0, 3, _lib.i64x3(a.shape), dp(A), dp(t), 32, 0.0, 1.0, 0.0, 1.0, None, dp(out)) == -1
    mn, mx = C.c_float(), C.c_float()
    assert lib.mvs_finite_range(0, None, 0, 10, C.byref(mn), C.byref(mx), C.byref(n)) == -1
    assert lib.mvs_finite_range(0, p, 0, 0, C.byref(mn), C.byref(mx), C.byref(n)) == -1
