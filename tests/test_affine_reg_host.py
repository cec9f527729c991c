"""CPU: the host side of affine_registration -- the numpy restatement (tests/affine_reg_oracle.py) recovers a known pose, the
per-sample header (csrc/mvs_affine_reg_dev.h) compiled for the host equals the restatement's float32 mode bit for bit, the
model algebra of _affine_reg.py (Jacobians, exponential updates) and the conversion of a pose between pyramid levels."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import affine_reg_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [((40, 48), m) for m in ao.MODELS] + [((20, 36, 44), m) for m in ("rigid", "similarity", "affine")]


@pytest.mark.parametrize("shape,model", CASES, ids=[f"{len(s)}d-{m}" for s, m in CASES])
@pytest.mark.parametrize("seed", [0, 3])
def test_oracle_recovers_the_known_pose(shape, model, seed):
    """Corner error <= 0.05 px (4x the largest value the algorithm's prototype measured on these inputs, 0.012 px, to allow for
    other numpy / scipy builds), and below the error of the same run without the gain / offset fit."""
    F, M, A0, t0 = ao.make_pair(shape, seed, model)
    out = ao.register(F, M, model)
    err = ao.corner_displacement(out["A"], out["t"], A0, t0, shape)
    plain = ao.register(F, M, model, fit_intensity=False)
    err_plain = ao.corner_displacement(plain["A"], plain["t"], A0, t0, shape)
    print(f"{shape} {model} seed {seed}: corner error {err:.4f} px, without intensity fit {err_plain:.4f} px, "
          f"{len(out['history'])} iterations")
    assert err <= 0.05
    assert err < err_plain


def _f32(tokens):
    return np.array([int(t, 16) for t in tokens], dtype=np.uint32).view(np.float32)


def _f64(tokens):
    return np.array([int(t, 16) for t in tokens], dtype=np.uint64).view(np.float64)


def test_header_samples_equal_the_oracle_float32_mode_bit_for_bit(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "affine_reg_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "affine_reg_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    rows = {k: [ln.split()[1:] for ln in lines if ln.startswith(k + " ")] for k in ("S3", "S2", "P", "C3", "C2")}
    assert len(rows["S3"]) == 600 and len(rows["S2"]) == 600 and len(rows["P"]) == 400 and len(rows["C3"]) == 300 and len(rows["C2"]) == 300

    for key, nd in (("S3", 3), ("S2", 2)):
        nt = 1 << nd
        tab = rows[key]
        taps = np.stack([_f32(row[:nt]) for row in tab], axis=-1).reshape((2,) * nd + (len(tab),))
        fr = [np.array([_f32([row[nt + k]])[0] for row in tab], dtype=np.float32) for k in range(nd)]
        ok = np.array([int(row[nt + nd]) for row in tab], dtype=bool)
        got = np.stack([_f32(row[nt + nd + 1:]) for row in tab])           # v, g...
        want_ok = np.isfinite(taps).reshape(nt, -1).all(axis=0)
        np.testing.assert_array_equal(ok, want_ok)
        assert 0 < (~ok).sum() < ok.size // 4
        with np.errstate(invalid="ignore", over="ignore"):
            v, g = ao.sample(taps, fr)
        want = np.stack([v] + g, axis=1)
        assert want.dtype == np.float32
        np.testing.assert_array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
        assert any((f == 0).any() for f in fr)

    p = _f64([row[0] for row in rows["P"]])
    n = np.array([int(row[1]) for row in rows["P"]])
    ok = np.array([int(row[2]) for row in rows["P"]], dtype=bool)
    i0 = np.array([int(row[3]) for row in rows["P"]])
    f = _f32([row[4] for row in rows["P"]])
    last_cell = 0
    for k in range(len(p)):
        w_ok, w_i0, w_f = ao.split(p[k:k + 1], int(n[k]), np.float32)
        assert bool(w_ok[0]) == bool(ok[k]), (p[k], n[k])
        if ok[k]:
            assert int(w_i0[0]) == i0[k] and w_f.view(np.uint32)[0] == f[k:k + 1].view(np.uint32)[0]
            assert 0 <= i0[k] and i0[k] + 1 <= n[k] - 1
            last_cell += int(i0[k] + 1 == n[k] - 1)
    assert last_cell >= 50 and (ok & (f == 0)).sum() >= 20 and (~ok).sum() >= 100

    for key, nd in (("C3", 3), ("C2", 2)):
        for row in rows[key]:
            vals = _f64(row)
            want = ao.coord(vals[:nd], list(vals[nd:2 * nd]), vals[2 * nd])
            assert np.float64(want).view(np.uint64) == vals[2 * nd + 1:].view(np.uint64)[0]


WALK_SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (127, 3), (128, 3), (129, 3), (257, 130), (3, 4, 130), (2, 129, 65)]


def test_walk_visits_every_valid_voxel_once_with_the_loop_values(tmp_path):
    """csrc/mvs_affine_walk_dev.h on the host: block_pos and walk_run called for every block, wave and lane reach exactly the
    voxels a plain loop over the crop finds valid, each once, with the loop's v, g and dy bit for bit.  The shapes are the
    smallest that reach every edge of the mapping: one voxel, 63 / 64 / 65 columns, 127 / 128 / 129 rows, three y chunks by three
    x blocks with partial last ones, and the same in 3D."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "affine_walk_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "affine_walk_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    lines = r.stdout.strip().splitlines()
    rows = [[int(t) for t in ln.split()[1:]] for ln in lines if ln.startswith("W ")]
    assert len(rows) == 2 * len(WALK_SHAPES)
    seen = set()
    for nd, nz, ny, nx, ipose, blocks, valid, visited, twice, missing, extra, differ in rows:
        shape = (nz, ny, nx)[3 - nd:]
        seen.add((shape, ipose))
        assert blocks == nz * -(-ny // 128) * -(-nx // 64), (shape, blocks)
        assert twice == 0, (shape, ipose, twice)
        assert missing == 0 and extra == 0 and visited == valid, (shape, ipose, valid, visited, missing, extra)
        assert differ == 0, (shape, ipose, differ)
        # not vacuous: a crop of one voxel has no interpolation cell; at the identity the cells clear of the last voxel of each axis
        # and of the NaN border take part unless one of their 1 + 2^ndim values is among the 2 % NaN voxels (17 % of them in 3D)
        cells = (nz - 1 if nd == 3 else 1) * (ny - (3 if ny >= 8 else 1)) * (nx - (3 if nx >= 8 else 1))
        assert valid > 0 or shape == (1, 1), (shape, ipose)
        assert ipose == 1 or cells // 2 <= valid <= cells, (shape, valid, cells)
    assert seen == {(s, p) for s in WALK_SHAPES for p in (0, 1)}
    assert r.returncode == 0 and lines[-1] == "done"


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("model", ao.MODELS)
def test_model_jacobian_is_the_derivative_of_the_update(model, ndim):
    from multiview_stitcher_amd import _affine_reg as ar

    rng = np.random.default_rng(5 + ndim)
    A, _ = ao.true_pose("affine", ndim, 1)
    t = rng.standard_normal(ndim)
    B = ar.model_jacobian(model, A)
    nq = ar.n_model_params(model, ndim)
    assert B.shape == (ndim * (ndim + 1), nq) and nq == ao.n_params(model, ndim)
    h = 1e-6
    for k in range(nq):
        e = np.zeros(nq)
        e[k] = h
        Ap, tp = ar.apply_update(model, A, t, e)
        Am, tm = ar.apply_update(model, A, t, -e)
        fd = (np.concatenate([Ap, tp[:, None]], axis=1) - np.concatenate([Am, tm[:, None]], axis=1)).ravel() / (2 * h)
        np.testing.assert_allclose(B[:, k], fd, atol=1e-9)
    np.testing.assert_allclose(B, ao.jacobian(model, A), atol=1e-15)
    # the update agrees with the restatement's matrix exponential
    q = 0.3 * rng.standard_normal(nq)
    A1, t1 = ar.apply_update(model, A, t, q)
    A2, t2 = ao.update(model, A, t, q)
    np.testing.assert_allclose(A1, A2, atol=1e-13)
    np.testing.assert_allclose(t1, t2, atol=1e-15)


@pytest.mark.parametrize("ndim", [2, 3])
def test_rigid_updates_keep_a_rotation_and_similarity_updates_a_scaled_one(ndim):
    from multiview_stitcher_amd import _affine_reg as ar

    rng = np.random.default_rng(11)
    A, t = np.eye(ndim), np.zeros(ndim)
    nq = ar.n_model_params("rigid", ndim)
    for _ in range(20):
        A, t = ar.apply_update("rigid", A, t, 0.5 * rng.standard_normal(nq))
    np.testing.assert_allclose(A.T @ A, np.eye(ndim), atol=1e-12)
    assert np.linalg.det(A) > 0
    A, t = ar.apply_update("similarity", A, t, 0.5 * rng.standard_normal(nq + 1))
    AtA = A.T @ A
    np.testing.assert_allclose(AtA, AtA[0, 0] * np.eye(ndim), atol=1e-12)
    assert abs(AtA[0, 0] - 1.0) > 1e-3


@pytest.mark.parametrize("shape", [(21, 37, 44), (41, 48)])
def test_level_conversion_with_odd_lengths(shape):
    """A pose converted to bin 2 and back is unchanged, and it maps the centre of a binned voxel to where the full-resolution
    pose maps that centre's full-resolution position (lengths that are no multiple of the bin: the trimmed grid is off centre)."""
    from multiview_stitcher_amd import _affine_reg as ar

    ndim, b = len(shape), 2
    A, t = ao.true_pose("affine", ndim, 2, t0=(2.5, -1.25, 0.75)[3 - ndim:])
    assert np.any(ar.level_offset(shape, b) != 0)
    np.testing.assert_array_equal(ar.level_offset(shape, b), ao.level_d(shape, b))
    tb = ar.to_level(A, t, shape, b)
    np.testing.assert_allclose(ar.from_level(A, tb, shape, b), t, atol=1e-13)
    np.testing.assert_allclose(tb, ao.to_level(A, t, shape, b), atol=1e-15)
    nb = np.array([n // b for n in shape])
    c, cb = (np.array(shape) - 1) / 2.0, (nb - 1) / 2.0
    rng = np.random.default_rng(0)
    for _ in range(20):
        j = rng.integers(0, nb)                       # a binned voxel; its centre in full-resolution pixels:
        x = b * j + (b - 1) / 2.0
        q = cb + tb + A @ (j - cb)                    # where the level pose maps it (binned px) ...
        p = c + t + A @ (x - c)                       # ... and the full-resolution pose (full px)
        np.testing.assert_allclose(b * q + (b - 1) / 2.0, p, atol=1e-11)


def test_bad_arguments_return_error_codes():
    """ndim outside {2, 3}, NULL pointers and non-positive shapes are refused before anything touches a device."""
    import ctypes as C

    from multiview_stitcher_amd import _lib

    lib = _lib.load()
    a = np.zeros((4, 5, 6), np.float32)
    A, t, out = np.eye(3), np.zeros(3), np.zeros(_lib.MVS_AFFINE_NEQ_LEN)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    call = lambda f, m, nd, shp: lib.mvs_affine_normal_eq(0, f, m, 0, nd, _lib.i64x3(shp), dp(A), dp(t), 1.0, 0.0, dp(out))
    assert call(a.ctypes.data, a.ctypes.data, 4, a.shape) == -1
    assert call(a.ctypes.data, a.ctypes.data, 1, a.shape) == -1
    assert call(None, a.ctypes.data, 3, a.shape) == -1
    assert call(a.ctypes.data, None, 3, a.shape) == -1
    assert call(a.ctypes.data, a.ctypes.data, 3, (4, 0, 6)) == -1
    assert call(a.ctypes.data, a.ctypes.data, 3, (-4, 5, 6)) == -1
    assert lib.mvs_affine_normal_eq(0, a.ctypes.data, a.ctypes.data, 0, 3, _lib.i64x3(a.shape), dp(A), dp(t), 1.0, 0.0, None) == -1


@pytest.mark.parametrize("shape,model", [((41, 48), "similarity"), ((21, 37, 44), "rigid")], ids=["2d-similarity", "3d-rigid"])
def test_host_loop_on_the_oracle_normal_equations_equals_the_oracle_loop(shape, model):
    """_affine_reg.optimise driven by the restatement's normal equations (no device) walks the restatement's iterations: the
    projection, the solve, the updates, the level conversion on odd lengths, the intensity fit and the stop rule agree."""
    from multiview_stitcher_amd import _affine_reg as ar

    F, M, A0, t0 = ao.make_pair(shape, 1, model)
    want = ao.register(F, M, model)
    bins = (2, 1)
    crops = [(ao.bin_mean(F, b), ao.bin_mean(M, b)) for b in bins]
    neq = lambda li, A, tb, gain, bias: ao.normal_equations(crops[li][0], crops[li][1], A, tb, gain, bias)   # noqa: E731
    nd = len(shape)
    A, t, history = ar.optimise(neq, bins, shape, model, np.eye(nd), np.zeros(nd), (30, 20), 1e-3, True)
    assert len(history) == len(want["history"])
    np.testing.assert_allclose(A, want["A"], atol=1e-9)
    np.testing.assert_allclose(t, want["t"], atol=1e-9)
    np.testing.assert_allclose([h["step"] for h in history], [h["step"] for h in want["history"]], rtol=1e-6, atol=1e-12)
    assert ao.corner_displacement(A, t, A0, t0, shape) <= 0.05
    np.testing.assert_allclose(ar.pose_to_matrix(A, t, shape), want["affine_matrix"], atol=1e-9)
    A2, t2 = ar.matrix_to_pose(ar.pose_to_matrix(A, t, shape), shape)
    np.testing.assert_allclose(t2, t, atol=1e-12)

    # refusals of the loop: too few samples, and a matrix that is not positive definite
    few = lambda *a: (np.eye(nd * (nd + 1)), np.zeros(nd * (nd + 1)), 0.0, 4 * ar.n_model_params(model, nd) - 1, (0.0,) * 5)   # noqa: E731
    with pytest.raises(ar.Refused):
        ar.optimise(few, (1,), shape, model, np.eye(nd), np.zeros(nd), (5,), 1e-3, True)
    flat = lambda *a: (np.zeros((nd * (nd + 1),) * 2), np.zeros(nd * (nd + 1)), 0.0, 1000, (0.0,) * 5)   # noqa: E731
    with pytest.raises(ar.Refused):
        ar.optimise(flat, (1,), shape, model, np.eye(nd), np.zeros(nd), (5,), 1e-3, True)
