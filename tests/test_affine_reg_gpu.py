"""GPU: mvs_affine_normal_eq against the numpy restatement (tests/affine_reg_oracle.py) -- valid counts exactly, sums within
a multiple of the restatement's own float32 / float64 deviation -- its determinism, affine_registration on crops against the
restatement's loop and the known pose, its default initialisation, its refusals, concurrent context lanes, and the
function as pairwise_reg_func of register() + fuse() on a view whose metadata rotation is wrong."""
import functools
import threading
import warnings

import numpy as np
import pytest
from scipy import ndimage

from tests import affine_reg_oracle as ao

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
CASES = [((40, 48), m) for m in ao.MODELS] + [((20, 36, 44), m) for m in ("rigid", "similarity", "affine")]
CASE_IDS = [f"{len(s)}d-{m}" for s, m in CASES]


# ---- 1. normal equations ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _neq_inputs(shape):
    F, M, _, _ = ao.make_pair(shape, 7, "affine")
    M = M.copy()
    for ax in (-2, -1):                    # a NaN border on y and x (on top of the three NaN columns make_pair leaves)
        idx = [slice(None)] * M.ndim
        for edge in (0, -1):
            idx[ax] = edge
            M[tuple(idx)] = np.nan
    nd = len(shape)
    rng = np.random.default_rng(42)
    A = np.eye(nd) + 0.02 * rng.standard_normal((nd, nd))
    t = 0.4 * rng.standard_normal(nd)
    F.setflags(write=False)
    M.setflags(write=False)
    return F, M, ((np.eye(nd), np.zeros(nd)), (A, t))


@functools.lru_cache(maxsize=None)
def _neq_reference(shape, ipose):
    F, M, poses = _neq_inputs(shape)
    A, t = poses[ipose]
    return ao.normal_equations(F, M, A, t, 1.05, -0.02, np.float64), ao.normal_equations(F, M, A, t, 1.05, -0.02, np.float32)


def _neq_errors(got, want):
    """Relative Frobenius error of H, error of b in units of its Cauchy-Schwarz bound sqrt(H_ii sum r^2), relative errors of
    sum r^2 and of the five moments."""
    H, b, sr2, n, mom = got
    H0, b0, sr20, n0, mom0 = want
    scale = np.sqrt(np.diag(H0) * sr20)
    e = {"H": np.linalg.norm(H - H0) / np.linalg.norm(H0), "b": float(np.max(np.abs(b - b0) / scale)), "sr2": abs(sr2 - sr20) / sr20}
    for name, a, a0 in zip(("sv", "sF", "svF", "sv2", "sF2"), mom, mom0):
        e[name] = abs(a - a0) / abs(a0)
    return e


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("ipose", [0, 1], ids=["identity", "affine"])
@pytest.mark.parametrize("shape", [(40, 48), (5, 6, 7), (21, 37, 44), (3, 4, 130), (130, 33), (3, 129, 65)], ids=str)
def test_normal_equations_match_the_oracle(hip_device, shape, ipose, mem):
    """Valid count: exact.  Every sum: within 8x the deviation of the restatement's float32 mode from its float64 mode on the
    same input (floor 16 eps32) -- the margin covers the kernel's float32 run sums of 32 samples and its summation tree.  The last
    two shapes have two chunks of rows with a partial second one; (3, 129, 65) also a second block of columns with one live lane."""
    from multiview_stitcher_amd import _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    F, M, poses = _neq_inputs(shape)
    A, t = poses[ipose]
    want64, want32 = _neq_reference(shape, ipose)
    if mem == "device":
        F, M = DeviceArray.from_host(F, hip_device), DeviceArray.from_host(M, hip_device)
    got = _reg_ops.affine_normal_equations(F, M, A, t, 1.05, -0.02, hip_device)
    assert want64[3] > 0 and want32[3] == want64[3]
    assert got[3] == want64[3]
    assert np.array_equal(got[0], got[0].T)
    err, dev = _neq_errors(got, want64), _neq_errors(want32, want64)
    ratios = {k: err[k] / max(dev[k], 2 * EPS32) for k in err}
    print(f"neq {shape} pose {ipose} {mem}: n = {int(got[3])}; error / max(float32-mode deviation, 2 eps32): "
          + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    for k in err:
        assert err[k] <= max(8 * dev[k], 16 * EPS32), (k, err[k], dev[k])


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------
def test_normal_equations_are_deterministic(hip_device):
    import ctypes as C

    from multiview_stitcher_amd import _lib
    from multiview_stitcher_amd.transformation import shape3

    lib = _lib.init(hip_device)
    for shape in [(40, 48), (21, 37, 44)]:
        F, M, poses = _neq_inputs(shape)
        nd = len(shape)
        A3, t3 = np.eye(3), np.zeros(3)
        A3[3 - nd:, 3 - nd:], t3[3 - nd:] = poses[1]
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
        outs = []
        for _ in range(2):
            out = np.full(_lib.MVS_AFFINE_NEQ_LEN, np.nan)
            rc = lib.mvs_affine_normal_eq(hip_device, F.ctypes.data, M.ctypes.data, _lib.MVS_MEM_HOST, nd, _lib.i64x3(shape3(shape)),
                                          dp(A3), dp(t3), 1.05, -0.02, dp(out))
            _lib.check(rc, hip_device, "mvs_affine_normal_eq")
            outs.append(out.tobytes())
        assert outs[0] == outs[1]
        assert np.isfinite(np.frombuffer(outs[0], dtype=np.float64)).all()


# ---- 3. / 4. end to end on crops ----------------------------------------------------------------------------------------------
def _contraction(history):
    """Ratio of the last two steps of the final level."""
    steps = [h["step"] for h in history if h["level"] == history[-1]["level"]]
    assert len(steps) >= 2
    return steps[-1] / steps[-2]


@functools.lru_cache(maxsize=None)
def _oracle_run(shape, model, seed):
    F, M, A0, t0 = ao.make_pair(shape, seed, model)
    out = ao.register(F, M, model, max_iterations=(60, 40), tolerance=1e-4)
    return F, M, A0, t0, out


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("shape,model", CASES, ids=CASE_IDS)
def test_registration_matches_the_oracle_loop_and_the_known_pose(hip_device, shape, model, seed):
    """Both loops stop within one tolerance of their common fixed point while the contraction factor is below one half (asserted
    on the restatement's step history): 4x tolerance between them leaves a margin of 2."""
    from multiview_stitcher_amd import registration

    tol = 1e-4
    F, M, A0, t0, want = _oracle_run(shape, model, seed)
    assert _contraction(want["history"]) < 0.5
    got = registration.affine_registration(F, M, transform_type=model, initial_affine="identity", tolerance=tol, max_iterations=(60, 40),
                                           device=hip_device, return_debug=True)
    A, t = ao.matrix_to_pose(got["affine_matrix"], shape)
    d = ao.corner_displacement(A, t, want["A"], want["t"], shape)
    err = ao.corner_displacement(A, t, A0, t0, shape)
    err_oracle = ao.corner_displacement(want["A"], want["t"], A0, t0, shape)
    print(f"e2e {shape} {model} seed {seed}: GPU vs oracle {d:.2e} px, vs truth {err:.4f} px (oracle {err_oracle:.4f}), "
          f"{len(got['debug']['history'])} / {len(want['history'])} iterations, quality {got['quality']:.4f}")
    assert d <= 4 * tol
    assert err <= err_oracle + 4 * tol
    assert got["quality"] > 0.9
    assert np.array_equal(got["debug"]["initial_affine"], np.eye(len(shape) + 1))


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("shape,model", CASES, ids=CASE_IDS)
def test_default_initialisation_from_phase_correlation(hip_device, shape, model, seed):
    """A shift of (6, -5, 4) px is outside the reach of the Gauss-Newton steps alone; the defaults start from the phase
    correlation's translation.  Compared with the restatement started from the same initial pose, bound as above.  The ratio of
    the restatement's last two steps is printed, not asserted: at the default tolerance of 1e-3 a run can stop before the
    asymptotic contraction (measured: 0.72 for 2d-affine seed 3)."""
    from multiview_stitcher_amd import registration

    nd = len(shape)
    F, M, A0, t0 = ao.make_pair(shape, seed, model, t0=(6.0, -5.0, 4.0)[:nd] if nd == 3 else (6.0, -5.0))
    got = registration.affine_registration(F, M, transform_type=model, device=hip_device, return_debug=True)
    init = got["debug"]["initial_affine"]
    assert np.array_equal(init[:nd, :nd], np.eye(nd)) and np.abs(init[:nd, nd]).max() > 3.0
    want = ao.register(F, M, model, initial_affine=init)
    tol = 1e-3
    A, t = ao.matrix_to_pose(got["affine_matrix"], shape)
    d = ao.corner_displacement(A, t, want["A"], want["t"], shape)
    err = ao.corner_displacement(A, t, A0, t0, shape)
    err_oracle = ao.corner_displacement(want["A"], want["t"], A0, t0, shape)
    print(f"default init {shape} {model} seed {seed}: initial shift {init[:nd, nd]}, GPU vs oracle {d:.2e} px, vs truth {err:.4f} px "
          f"(oracle {err_oracle:.4f}), ratio of the restatement's last two steps {_contraction(want['history']):.2f}")
    assert d <= 4 * tol
    assert err <= err_oracle + 4 * tol


# ---- 5. through register() -----------------------------------------------------------------------------------------------------
def _rot3(deg_yx, deg_zx=0.0):
    a, b = np.deg2rad(deg_yx), np.deg2rad(deg_zx)
    ryx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rzx = np.array([[np.cos(b), 0, -np.sin(b)], [0, 1, 0], [np.sin(b), 0, np.cos(b)]])
    return ryx @ rzx


def _about(lin, centre, shift=(0.0, 0.0, 0.0)):
    m = np.eye(4)
    m[:3, :3] = lin
    m[:3, 3] = centre - lin @ centre + np.asarray(shift)
    return m


def _rotated_pair(seed=3):
    """Two views (32 x 64 x 64, unit spacing) of one smooth volume.  View 1 sits on the world grid; view 2 is rotated by 5 deg
    about z and tilted by 1 deg.  View 2's metadata is wrong by a rotation of 1.5 deg about the view's centre plus a shift."""
    from multiview_stitcher_amd import spatial_image_utils as si

    rng = np.random.default_rng(seed)
    G = ndimage.gaussian_filter(rng.random((56, 104, 128)), 2.0).astype(np.float32)
    G = (G - G.min()) / (G.max() - G.min())
    n = (32, 64, 64)
    o1, o2 = np.array([12.0, 20.0, 14.0]), np.array([12.0, 20.0, 46.0])
    v1 = G[tuple(slice(int(o), int(o) + k) for o, k in zip(o1, n))].copy()
    centre2 = o2 + (np.array(n) - 1) / 2.0
    A2 = _about(_rot3(5.0, 1.0), centre2)
    # view 2 voxel p holds G(A2 @ (o2 + p))
    v2 = ndimage.affine_transform(G, A2[:3, :3], offset=A2[:3, :3] @ o2 + A2[:3, 3], output_shape=n, order=3, mode="nearest").astype(np.float32)
    A2_meta = _about(_rot3(1.5), A2[:3, :3] @ centre2 + A2[:3, 3], shift=(0.8, -1.4, 1.1)) @ A2
    sims = []
    for data, o, A in ((v1, o1, np.eye(4)), (v2, o2, A2_meta)):
        s = si.to_spatial_image(data, dims=["z", "y", "x"], scale=dict(zip("zyx", np.ones(3))), translation=dict(zip("zyx", o)))
        si.set_sim_affine(s, A, "stage")
        sims.append(s)
    corners = np.array([[o2[k] + (n[k] - 1) * (bits >> k & 1) for k in range(3)] for bits in range(8)])
    return sims, A2, A2_meta, G, corners


def _worst_corner_error(P, A2, corners):
    return max(float(np.linalg.norm((P[:3, :3] @ c + P[:3, 3]) - (A2[:3, :3] @ c + A2[:3, 3]))) for c in corners)


def test_register_with_affine_registration_removes_a_rotation_error_and_fuses(hip_device):
    from multiview_stitcher_amd import fusion, param_utils, registration
    from multiview_stitcher_amd import spatial_image_utils as si

    errs = {}
    for name, kwargs in (("phase_correlation", {}),
                         ("affine_registration", {"pairwise_reg_func": registration.affine_registration,
                                                  "pairwise_reg_func_kwargs": {"transform_type": "rigid"}})):
        sims, A2, A2m, G, corners = _rotated_pair()
        registration.register(sims, transform_key="stage", new_transform_key="reg", device=hip_device,
                              groupwise_resolution_kwargs={"transform": "rigid", "reference_view": 0}, **kwargs)
        p1 = param_utils.select_time(si.get_affine_from_sim(sims[0], "reg"), 0)
        p2 = param_utils.select_time(si.get_affine_from_sim(sims[1], "reg"), 0)
        np.testing.assert_allclose(p1, np.eye(4), atol=1e-9)
        errs[name] = _worst_corner_error(p2, A2, corners)
    before = _worst_corner_error(A2m, A2, corners)
    print(f"register(): worst corner error of view 2: metadata {before:.3f} px, phase correlation {errs['phase_correlation']:.3f} px, "
          f"affine_registration {errs['affine_registration']:.4f} px")
    assert before > 1.5
    assert errs["affine_registration"] < errs["phase_correlation"]
    assert errs["affine_registration"] <= 0.05 + 4e-3          # 4x the default tolerance, the bound of the crop tests

    fused = fusion.fuse(sims, transform_key="reg", output_chunksize={"z": 64, "y": 64, "x": 64})
    f = np.asarray(fused.data, dtype=np.float64).squeeze()
    o = si.get_origin_from_sim(fused, asarray=True)
    sp = si.get_spacing_from_sim(fused, asarray=True)
    want = ndimage.affine_transform(G.astype(np.float64), np.diag(sp), offset=o, output_shape=f.shape, order=1, mode="constant", cval=np.nan)
    inner = tuple(slice(6, -6) for _ in range(3))
    m = ~np.isnan(want[inner]) & (f[inner] > 0)
    assert m.mean() > 0.5
    assert np.abs(f[inner][m] - want[inner][m]).mean() < 0.01          # data range is [0, 1]; residual = resampling blur


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_device):
    from multiview_stitcher_amd import registration

    F, M, _, _ = ao.make_pair((20, 36, 44), 0, "rigid")
    sparse = np.full_like(M, np.nan)
    sparse[10, 18, 20:30] = M[10, 18, 20:30]
    with pytest.warns(UserWarning, match="affine_registration"):
        got = registration.affine_registration(F, sparse, device=hip_device, return_debug=True)
    assert np.isnan(got["quality"])
    assert np.array_equal(got["affine_matrix"], got["debug"]["initial_affine"])

    const = np.full_like(F, 0.25)
    with pytest.warns(UserWarning, match="constant"):
        got = registration.dispatch_pairwise_reg_func(registration.affine_registration, fixed_data=const, moving_data=M, device=hip_device,
                                                      transform_type="rigid")
    assert np.isnan(got["quality"]) and np.array_equal(got["affine_matrix"], np.eye(4))


# ---- 7. context lanes -------------------------------------------------------------------------------------------------------------
def test_two_lanes_at_once_equal_the_serial_results(hip_device):
    from multiview_stitcher_amd import registration

    jobs = [(ao.make_pair((20, 36, 44), 0, "rigid")[:2], "rigid"), (ao.make_pair((40, 48), 3, "affine")[:2], "affine")]
    run = lambda job, dev: registration.affine_registration(job[0][0], job[0][1], transform_type=job[1], device=dev, return_debug=True)
    serial = [run(job, hip_device) for job in jobs]
    results, errors = [None, None], []
    barrier = threading.Barrier(2)

    def work(k):
        try:
            barrier.wait(timeout=60)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
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
        assert got["affine_matrix"].tobytes() == want["affine_matrix"].tobytes()
        assert np.float64(got["quality"]).tobytes() == np.float64(want["quality"]).tobytes()
        assert [h["step"] for h in got["debug"]["history"]] == [h["step"] for h in want["debug"]["history"]]
