"""GPU: mvs_affine_joint_hist and mvs_affine_mi_gradient against the numpy restatement (tests/affine_mi_oracle.py) -- the
histogram as integers, the gradient sums within a multiple of the restatement's own float32 / float64 deviation -- their
determinism, alone and on two context lanes at once, affine_registration(metric="mattes") on crops against the restatement's
loop and the known pose, through register() on a remapped and rotated tile, its refusal of a constant crop, and the default
metric's unchanged bits."""
import functools
import threading
import warnings

import numpy as np
import pytest
from scipy import ndimage

from tests import affine_mi_oracle as mo
from tests import affine_reg_oracle as ao

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
# the smallest shapes that still cross a block's 64 x columns, a run's 128 rows and the one-block case
SHAPES = [(5, 64), (37, 70), (130, 33), (3, 9, 33), (6, 21, 130)]
BINS = (8, 32, 64)


# ---- the inputs the kernel tests share -------------------------------------------------------------------------------------
def _poses(shape):
    """Identity, and a rotation + shear + shift that moves about a third of the samples out of the moving crop."""
    nd = len(shape)
    a = 0.05
    A = np.eye(nd)
    A[nd - 2:, nd - 2:] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    A[nd - 2, nd - 1] += 0.04
    if nd == 3:
        A[0, 2] += 0.004
        A[1, 0] -= 0.03
    t = np.array([0.1, 0.12 * shape[-2] + 0.3, -0.2 * shape[-1] - 0.4][3 - nd:])
    return (np.eye(nd), np.zeros(nd)), (A, t)


def _inside_fraction(shape, A, t):
    p, _ = ao.coordinates(shape, A, t)
    inside = np.ones(shape, dtype=bool)
    for k in range(len(shape)):
        inside &= (p[k] >= 0) & (p[k] < shape[k] - 1)
    return float(inside.mean())


@functools.lru_cache(maxsize=None)
def _inputs(shape, nan):
    """A smooth scene and its remapped, slightly moved image.  ``nan``: a 2-voxel NaN frame on y and x of the fixed crop (the z
    axes here are too short for one) and a NaN block in the moving crop."""
    F, M, _, _ = mo.make_pair(shape, 11, "rigid", sigma=2.0)
    if nan:
        F, M = F.copy(), M.copy()
        for ax in (-2, -1):
            idx = [slice(None)] * F.ndim
            for edge in (slice(0, 2), slice(-2, None)):
                idx[ax] = edge
                F[tuple(idx)] = np.nan
        M[..., shape[-2] // 3:shape[-2] // 3 + 2, shape[-1] // 2:shape[-1] // 2 + 7] = np.nan
    F.setflags(write=False)
    M.setflags(write=False)
    return F, M


@functools.lru_cache(maxsize=None)
def _hist_reference(shape, nan, ipose, B):
    F, M = _inputs(shape, nan)
    rng = mo.ranges(F, M, B)
    A, t = _poses(shape)[ipose]
    return rng, mo.joint_hist(F, M, A, t, B, rng, np.float32)


def _on(mem, hip_device, *arrays):
    from multiview_stitcher_amd.device import DeviceArray

    return [DeviceArray.from_host(a, hip_device) for a in arrays] if mem == "device" else list(arrays)


def test_the_second_pose_moves_about_a_third_of_the_samples_outside():
    for shape in SHAPES:
        (A0, t0), (A, t) = _poses(shape)
        base, moved = _inside_fraction(shape, A0, t0), _inside_fraction(shape, A, t)
        print(f"{shape}: inside the moving crop at identity {base:.2f}, at the second pose {moved:.2f}")
        assert base - moved > 0.15 and moved > 0.3


# ---- 1. histogram ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("ipose", [0, 1], ids=["identity", "moved"])
@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_joint_histogram_equals_the_oracle_as_integers(hip_device, shape, nan, ipose, B, mem):
    from multiview_stitcher_amd import _reg_ops

    F, M = _inputs(shape, nan)
    A, t = _poses(shape)[ipose]
    rng, (want, n_want) = _hist_reference(shape, nan, ipose, B)
    Fd, Md = _on(mem, hip_device, F, M)
    got, n = _reg_ops.affine_joint_hist(Fd, Md, A, t, B, rng, hip_device)
    assert n_want > 0 and n == n_want
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert abs(int(got.sum()) - n * 2 ** 20) <= 2 * n
    # the ranges the host passes are the restatement's
    lo_hi = _reg_ops.finite_range(Fd, hip_device), _reg_ops.finite_range(Md, hip_device)
    assert lo_hi[0][:2] == mo.finite_range(F) and lo_hi[1][:2] == mo.finite_range(M)
    assert lo_hi[0][2] == int(np.isfinite(F).sum()) and lo_hi[1][2] == int(np.isfinite(M).sum())


# ---- 2. gradient -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gradient_reference(shape, nan, ipose, B):
    """(table float32, sums of the float32 mode, sums of the float64 mode, Cauchy-Schwarz scale of every sum)."""
    F, M = _inputs(shape, nan)
    A, t = _poses(shape)[ipose]
    rng, (hist, _) = _hist_reference(shape, nan, ipose, B)
    table = mo.mutual_information(hist)[1].astype(np.float32)
    want32, n = mo.gradient_sums(F, M, A, t, B, rng, table, np.float32)
    want64, n64 = mo.gradient_sums(F, M, A, t, B, rng, table, np.float64)
    w, g, xt = mo.gradient_samples(F, M, A, t, B, rng, table, np.float64)
    nd = len(g)
    scale = np.array([np.sqrt(np.sum((g[k] * xt[m]) ** 2) * np.sum(w * w)) for k in range(nd) for m in range(nd + 1)])
    return table, want32, want64, scale, n


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("ipose", [0, 1], ids=["identity", "moved"])
@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradient_sums_match_the_oracle(hip_device, shape, nan, ipose, B, mem):
    """The bound tests/test_affine_reg_gpu.py applies to J^T r, for the same accumulation scheme: the error of every sum in units
    of its Cauchy-Schwarz bound sqrt(sum (g_k x_m)^2 sum w^2) is within 8x the deviation of the restatement's float32 mode from
    its float64 mode on the same input (floor 16 eps32, the reach of a float32 run sum of 32 samples).  Measured: at most 0.07
    eps32 over the 120 cases; the deviation of the float32 mode is 0.04 to 7 eps32, and thousands where a sample changes its bin
    between the two modes."""
    from multiview_stitcher_amd import _reg_ops

    F, M = _inputs(shape, nan)
    A, t = _poses(shape)[ipose]
    rng = _hist_reference(shape, nan, ipose, B)[0]
    table, want32, want64, scale, n_want = _gradient_reference(shape, nan, ipose, B)
    Fd, Md = _on(mem, hip_device, F, M)
    got, n = _reg_ops.affine_mi_gradient(Fd, Md, A, t, B, rng, table.reshape(B, B), hip_device)
    assert n == n_want and np.abs(want32).max() > 0
    ok = scale > 0          # a single valid row sits at y - c = 0: those sums are exact zeros
    assert ok.sum() >= len(shape) and np.all(got[~ok] == 0) and np.all(want32[~ok] == 0)
    err = float(np.max(np.abs(got - want32)[ok] / scale[ok]))
    dev = float(np.max(np.abs(want32 - want64)[ok] / scale[ok]))
    print(f"gradient {shape} nan {nan} pose {ipose} B {B} {mem}: n = {n}; error {err / EPS32:.2f} eps32, float32-mode deviation "
          f"{dev / EPS32:.2f} eps32")
    assert err <= max(8 * dev, 16 * EPS32), (err, dev)


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------
def _both_kernels(shape, B, device):
    from multiview_stitcher_amd import _reg_ops

    F, M = _inputs(shape, True)
    A, t = _poses(shape)[1]
    rng = _hist_reference(shape, True, 1, B)[0]
    table = _gradient_reference(shape, True, 1, B)[0]
    hist, n = _reg_ops.affine_joint_hist(F, M, A, t, B, rng, device)
    sums, n2 = _reg_ops.affine_mi_gradient(F, M, A, t, B, rng, table.reshape(B, B), device)
    return hist.tobytes() + sums.tobytes() + bytes([n == n2])


def test_two_calls_are_equal_bit_for_bit_alone_and_on_two_lanes_at_once(hip_device):
    jobs = [((6, 21, 130), 32), ((37, 70), 64)]
    serial = [_both_kernels(shape, B, hip_device) for shape, B in jobs]
    assert serial == [_both_kernels(shape, B, hip_device) for shape, B in jobs]
    results, errors = [None, None], []
    barrier = threading.Barrier(2)

    def work(k):
        try:
            barrier.wait(timeout=60)
            results[k] = [_both_kernels(*jobs[k], hip_device | (k + 1) << 8) for _ in range(3)]
        except BaseException as e:          # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for got, want in zip(results, serial):
        assert got == [want] * 3


# ---- 4. the loop on crops -------------------------------------------------------------------------------------------------------
def _loop_pair(nd):
    if nd == 2:      # the pair of tests/test_affine_mi_host.py
        a = 0.06
        A0 = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        return mo.make_pair((64, 64), 1, "rigid", sigma=3.0, A0=A0, t0=np.array([1.7, -2.3]))
    return mo.make_pair((24, 40, 40), 1, "rigid", sigma=3.0)


@functools.lru_cache(maxsize=None)
def _oracle_loop(nd, model):
    F, M, A0, t0 = _loop_pair(nd)
    return F, M, A0, t0, mo.register(F, M, model)


@pytest.mark.parametrize("model", ["rigid", "affine"])
@pytest.mark.parametrize("nd", [2, 3], ids=["2d", "3d"])
def test_registration_matches_the_oracle_loop_and_the_known_pose(hip_device, nd, model):
    """Acceptance as in tests/test_affine_reg_gpu.py: the error against the truth within 4x tolerance of the restatement's, and
    the pose within 4x tolerance of the restatement's.  The histograms of equal poses are equal integers, so both loops take the
    same decisions until the poses differ by the rounding of the gradient sums.  Measured: the two poses 2e-9 to 2e-7 px
    apart, history rows (both levels, the closing row of a level included) 14 (2d rigid), 19 (2d affine), 13 (3d rigid), 8 (3d
    affine) in both loops."""
    from multiview_stitcher_amd import registration

    tol = 1e-3
    F, M, A0, t0, want = _oracle_loop(nd, model)
    shape = F.shape
    got = registration.affine_registration(F, M, transform_type=model, initial_affine="identity", metric="mattes", tolerance=tol,
                                           device=hip_device, return_debug=True)
    A, t = ao.matrix_to_pose(got["affine_matrix"], shape)
    d = ao.corner_displacement(A, t, want["A"], want["t"], shape)
    err = ao.corner_displacement(A, t, A0, t0, shape)
    err_oracle = ao.corner_displacement(want["A"], want["t"], A0, t0, shape)
    hist = got["debug"]["history"]
    print(f"mattes {shape} {model}: GPU vs oracle {d:.2e} px, vs truth {err:.4f} px (oracle {err_oracle:.4f}), "
          f"{len(hist)} / {len(want['history'])} iterations, quality {got['quality']:.4f} (oracle {want['quality']:.4f})")
    assert set(hist[0]) == {"level", "mi", "n", "alpha", "step"}
    assert d <= 4 * tol
    assert err <= err_oracle + 4 * tol
    assert err <= 0.05
    assert 0.0 < got["quality"] <= 1.0 and abs(got["quality"] - want["quality"]) < 1e-3
    assert np.array_equal(got["debug"]["initial_affine"], np.eye(nd + 1))
    # the default metric does not solve this pair: the case needs the feature
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        ssd = registration.affine_registration(F, M, transform_type=model, initial_affine="identity", device=hip_device)
    assert ao.corner_displacement(*ao.matrix_to_pose(ssd["affine_matrix"], shape), A0, t0, shape) > 1.0


# ---- 5. through register() ------------------------------------------------------------------------------------------------------
def _remapped_rotated_pair(seed=5):
    """Two tiles (24 x 48 x 48, unit spacing) cut from one smooth scene, a third of a tile apart along x.  Tile 2 is rotated by
    0.03 rad about z through its centre and its intensities are remapped by |2 v - 2 median(v)|; its metadata knows only its
    position."""
    from multiview_stitcher_amd import spatial_image_utils as si

    rng = np.random.default_rng(seed)
    G = ndimage.gaussian_filter(rng.random((40, 80, 104)), 2.0).astype(np.float32)
    G = (G - G.min()) / (G.max() - G.min())
    n = (24, 48, 48)
    o1, o2 = np.array([8.0, 16.0, 14.0]), np.array([8.0, 16.0, 30.0])
    v1 = G[tuple(slice(int(o), int(o) + k) for o, k in zip(o1, n))].copy()
    a = 0.03
    R = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    centre2 = o2 + (np.array(n) - 1) / 2.0
    A2 = np.eye(4)
    A2[:3, :3] = R
    A2[:3, 3] = centre2 - R @ centre2
    # tile 2 voxel p holds G(A2 @ (o2 + p))
    v2 = ndimage.affine_transform(G, R, offset=R @ o2 + A2[:3, 3], output_shape=n, order=3, mode="nearest")
    sims = []
    for data, o in ((v1, o1), (mo.remap(v2), o2)):
        s = si.to_spatial_image(data, dims=["z", "y", "x"], scale=dict(zip("zyx", np.ones(3))), translation=dict(zip("zyx", o)))
        si.set_sim_affine(s, np.eye(4), "stage")
        sims.append(s)
    corners = np.array([[o2[k] + (n[k] - 1) * (bits >> k & 1) for k in range(3)] for bits in range(8)])
    return sims, A2, corners


def _worst_corner_error(P, A2, corners):
    return max(float(np.linalg.norm((P[:3, :3] @ c + P[:3, 3]) - (A2[:3, :3] @ c + A2[:3, 3]))) for c in corners)


def test_register_with_the_mattes_metric_aligns_a_remapped_rotated_tile(hip_device):
    """Both metrics start from the metadata (``initial_affine="identity"``): a phase correlation across this intensity relation
    finds no usable shift.  The restatement's loop on the same overlap (32 px) ends 0.009 px from the truth at the tile's
    corners.  Measured: 1.00 px before, 9.25 px with the default metric, 0.009 px with mattes."""
    from multiview_stitcher_amd import param_utils, registration
    from multiview_stitcher_amd import spatial_image_utils as si

    errs = {}
    for metric in ("ssd", "mattes"):
        sims, A2, corners = _remapped_rotated_pair()
        kwargs = {"transform_type": "rigid", "initial_affine": "identity"}
        if metric == "mattes":
            kwargs["metric"] = "mattes"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            registration.register(sims, transform_key="stage", new_transform_key="reg", device=hip_device,
                                  pairwise_reg_func=registration.affine_registration, pairwise_reg_func_kwargs=kwargs,
                                  groupwise_resolution_kwargs={"transform": "rigid", "reference_view": 0})
        p1 = param_utils.select_time(si.get_affine_from_sim(sims[0], "reg"), 0)
        p2 = param_utils.select_time(si.get_affine_from_sim(sims[1], "reg"), 0)
        np.testing.assert_allclose(p1, np.eye(4), atol=1e-9)
        errs[metric] = _worst_corner_error(p2, A2, corners)
    before = _worst_corner_error(np.eye(4), A2, corners)
    print(f"register(): worst corner error of tile 2: metadata {before:.3f} px, default metric {errs['ssd']:.3f} px, "
          f"mattes {errs['mattes']:.4f} px")
    assert before > 0.9
    assert errs["mattes"] < errs["ssd"]
    assert errs["mattes"] <= 0.05 + 4e-3          # the bound of the crop tests: 0.05 px + 4x the default tolerance


# ---- 6. refusals, 7. the default path ---------------------------------------------------------------------------------------------
def test_a_constant_moving_crop_is_refused(hip_device):
    from multiview_stitcher_amd import registration

    F, M, _, _ = _loop_pair(3)
    const = np.full_like(M, 0.25)
    const[:, :2] = np.nan
    with pytest.warns(UserWarning, match="affine_registration"):
        got = registration.affine_registration(F, const, metric="mattes", initial_affine="identity", device=hip_device, return_debug=True)
    assert np.isnan(got["quality"])
    assert np.array_equal(got["affine_matrix"], got["debug"]["initial_affine"]) and np.array_equal(got["affine_matrix"], np.eye(4))
    assert got["debug"]["history"] == []


def test_the_default_metric_returns_the_same_bits_as_no_metric(hip_device):
    from multiview_stitcher_amd import registration

    for shape, model in (((20, 36, 44), "rigid"), ((40, 48), "affine")):
        F, M, _, _ = ao.make_pair(shape, 3, model)
        a = registration.affine_registration(F, M, transform_type=model, device=hip_device, return_debug=True)
        b = registration.affine_registration(F, M, transform_type=model, device=hip_device, return_debug=True, metric="ssd", n_bins=16)
        assert a["affine_matrix"].tobytes() == b["affine_matrix"].tobytes()
        assert np.float64(a["quality"]).tobytes() == np.float64(b["quality"]).tobytes()
        assert a["debug"]["history"] == b["debug"]["history"] and set(a["debug"]["history"][0]) == {"level", "msd", "n", "gain", "bias", "step"}
