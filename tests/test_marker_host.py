"""CPU: the host side of registration.registration_marker_based -- argument validation (before any device is touched), the
RANSAC sample sets, the candidate de-duplication, the model fits, the point-set seam.  No test here initialises a device."""
import itertools
import warnings

import numpy as np
import pytest

from multiview_stitcher_amd import _marker_reg as mr
from multiview_stitcher_amd import msi_utils, registration
from multiview_stitcher_amd import spatial_image_utils as si
from tests import marker_oracle as mo

RNG = np.random.default_rng(11)
PTS3 = RNG.uniform(0, 50, (12, 3))
PTS2 = RNG.uniform(0, 50, (12, 2))

# (keyword overrides, fixed, moving, the reference's message)
BAD = [
    ({}, np.zeros(5), PTS3, "Marker point arrays must be two-dimensional."),
    ({}, PTS3, np.zeros((4, 3, 1)), "Marker point arrays must be two-dimensional."),
    ({}, PTS3, PTS2, "Fixed and moving marker points must have the same dimensionality."),
    ({}, np.zeros((0, 3)), PTS3, "Marker point arrays must not be empty."),
    ({}, PTS3, np.zeros((0, 3)), "Marker point arrays must not be empty."),
    ({"num_neighbors": 0}, PTS3, PTS3, "num_neighbors must be at least 1."),
    ({"redundancy": -1}, PTS3, PTS3, "redundancy must be non-negative."),
    ({"descriptor_ratio": 0.0}, PTS3, PTS3, "descriptor_ratio must be positive."),
    ({"descriptor_threshold_scale": -0.5}, PTS3, PTS3, "descriptor_threshold_scale must be non-negative."),
    ({"ransac_max_error": 0.0}, PTS3, PTS3, "ransac_max_error must be positive."),
    ({"ransac_num_iterations": 0}, PTS3, PTS3, "ransac_num_iterations must be at least 1."),
    ({"icp_max_error": 0.0}, PTS3, PTS3, "icp_max_error must be positive."),
    ({"icp_num_iterations": 0}, PTS3, PTS3, "icp_num_iterations must be at least 1."),
    ({"icp_tolerance": -1e-3}, PTS3, PTS3, "icp_tolerance must be non-negative."),
    ({"transform_type": "similarity"}, PTS3, PTS3,
     "Unsupported marker registration transform_type 'similarity'. Expected 'translation', 'rigid', or 'affine'."),
    ({"descriptor_distance_threshold": -1.0}, PTS3, PTS3, "descriptor_distance_threshold must be non-negative."),
    ({}, PTS3[:4], PTS3, "Not enough points to build marker descriptors. Need at least 5, got 4."),
    ({"num_neighbors": 2, "redundancy": 0}, PTS2, PTS2[:2], "Not enough points to build marker descriptors. Need at least 3, got 2."),
]


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Any attempt to initialise the library fails the test."""
    from multiview_stitcher_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "init", refuse)


@pytest.mark.parametrize("kw,fixed,moving,message", BAD, ids=[f"{i}-{b[3][:28]}" for i, b in enumerate(BAD)])
def test_validation_raises_the_reference_message_or_warns_and_returns_identity(kw, fixed, moving, message):
    with pytest.raises(ValueError) as e:
        registration.registration_marker_based(fixed, moving, **kw)
    assert str(e.value) == message
    with pytest.warns(UserWarning) as w:
        res = registration.registration_marker_based(fixed, moving, fail_on_error=False, **kw)
    assert [str(x.message) for x in w] == [message]
    ndim = fixed.shape[1] if fixed.ndim == 2 else (moving.shape[1] if moving.ndim == 2 else 2)
    assert np.array_equal(res["affine_matrix"], np.eye(ndim + 1)) and np.isnan(res["quality"])


def test_signature_is_the_reference_signature_plus_device():
    import inspect

    sig = inspect.signature(registration.registration_marker_based)
    want = [("fixed_points", inspect.Parameter.empty), ("moving_points", inspect.Parameter.empty), ("transform_type", "rigid"),
            ("num_neighbors", 3), ("redundancy", 1), ("descriptor_ratio", 3.0), ("descriptor_distance_threshold", None),
            ("descriptor_threshold_scale", 1.0), ("ransac_max_error", 5.0), ("ransac_min_inlier_ratio", 0.1),
            ("ransac_min_inlier_factor", 3.0), ("ransac_num_iterations", 1000), ("icp", False), ("icp_max_error", None),
            ("icp_num_iterations", 50), ("icp_tolerance", 1e-6), ("random_state", 0), ("fail_on_error", True), ("device", 0)]
    assert [(n, p.default) for n, p in sig.parameters.items()] == want


@pytest.mark.parametrize("kw,name", [({"num_neighbors": 6}, "num_neighbors"), ({"num_neighbors": 3, "redundancy": 12}, "redundancy"),
                                     ({"num_neighbors": 3, "redundancy": 3}, "redundancy")])
def test_parameters_beyond_the_kernels_are_refused_by_name(kw, name):
    pts = RNG.uniform(0, 50, (40, 3))
    with pytest.raises(NotImplementedError, match=name):
        registration.registration_marker_based(pts, pts, **kw)
    with pytest.raises(NotImplementedError, match=name):      # not a registration failure: fail_on_error does not swallow it
        registration.registration_marker_based(pts, pts, fail_on_error=False, **kw)


@pytest.mark.parametrize("n_cand,m,n_iter", [(36, 1, 1000), (12, 3, 1000), (13, 3, 285), (13, 3, 286), (60, 3, 1000), (60, 4, 50), (5, 4, 3)])
@pytest.mark.parametrize("state", ["int", "generator"])
def test_ransac_sample_sets_equal_the_oracle(n_cand, m, n_iter, state):
    """Exhaustive (comb <= iterations, the boundary 286 = C(13, 3) included) and random branch; an int seed and a Generator."""
    mk = (lambda: 5) if state == "int" else (lambda: np.random.default_rng(5))
    got = mr.ransac_samples(n_cand, m, n_iter, mk())
    want = mo.ransac_sample_sets(n_cand, m, n_iter, mk())
    assert got.shape == (len(want), m) and np.array_equal(got, np.asarray(want))


def _knn_tables(seed, n_fixed=30, n_moving=33):
    f, m, _ = mo.make_pair(3, n_fixed, seed, box=60.0, n_outliers=3, drop=0.0)
    tables = mo.descriptor_knn(mo.get_descriptors(f, 3, 1), mo.get_descriptors(m[:n_moving], 3, 1))
    return tables, mo.get_descriptor_distance_threshold(f, m, 3, 1.0)


@pytest.mark.parametrize("ratio,scale", [(3.0, 1.0), (1.2, 3.0), (1.0, 100.0)])
def test_candidate_deduplication_reproduces_the_oracle_order_included(ratio, scale):
    (dist, idx, fpi, mpi), thr = _knn_tables(3)
    # a descriptor whose neighbours all belong to ONE moving point: the second best is +inf, the ratio test passes
    dist, idx = dist.copy(), idx.copy()
    one_point = np.flatnonzero(mpi == mpi[idx[4, 0]])
    idx[4, :] = np.resize(one_point, idx.shape[1])
    dist[4, :] = np.sort(dist[4, :]) * 1e-3
    assert len(set(mpi[idx[4]])) == 1
    # and a pair proposed twice, the second time with the smaller distance (the reference keeps the FIRST position)
    idx[9], dist[9] = idx[8], dist[8] * 0.5
    fpi = fpi.copy()
    fpi[9] = fpi[8]
    want = mo.candidates_from_knn(dist, idx, fpi, mpi, ratio, thr * scale)
    got = mr.candidates_from_knn(dist, idx, fpi, mpi, ratio, thr * scale)
    assert len(want) > 3 and [fpi[4], mpi[idx[4, 0]]] in want.tolist()
    assert got.dtype == want.dtype and np.array_equal(got, want)
    empty = mr.candidates_from_knn(dist, idx, fpi, mpi, ratio, 0.0)
    assert empty.shape == (0, 2) and np.array_equal(empty, mo.candidates_from_knn(dist, idx, fpi, mpi, ratio, 0.0))


def test_neighbor_table_removes_self_by_index():
    """With duplicate points the first hit of a self query need not be the point itself (registration.py:667-671)."""
    idx = np.array([[1, 0, 2, 3], [0, 1, 3, 2], [2, 0, 1, 3], [0, 1, 2, 4]])
    got = mr.neighbor_table(idx, 2)
    want = [[int(i) for i in row if int(i) != p][:2] for p, row in enumerate(idx)]
    assert got.tolist() == want == [[1, 2], [0, 3], [0, 1], [0, 1]]


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("transform_type", ["translation", "rigid", "affine"])
def test_fits_equal_the_oracle(ndim, transform_type):
    f, _, true = mo.make_pair(ndim, 30, 21 + ndim)
    rng = np.random.default_rng(2)
    m = mo.transform_pts(f, true) + rng.normal(0.0, 0.1, f.shape)      # row i of m belongs to row i of f
    need = mo.get_min_matches(transform_type, ndim)
    samples = np.array([rng.choice(30, size=need, replace=False) for _ in range(20)])
    for size in (need, 12):      # minimal samples and an overdetermined set
        sets = samples if size == need else np.array([rng.choice(30, size=size, replace=False) for _ in range(5)])
        batch, valid = mr.fit_transforms_batch(f[sets], m[sets], transform_type)
        assert valid.all()
        for s, b in zip(sets, batch):
            want = mo.fit_transform(f[s], m[s], transform_type)
            one = mr.fit_transform(f[s], m[s], transform_type)
            assert np.array_equal(one, want)                     # the same float64 fit written twice
            scale = np.abs(mo.transform_pts(f, want)).max()
            assert np.abs(mo.transform_pts(f, b) - mo.transform_pts(f, want)).max() <= 1e-9 * scale


def test_degenerate_samples_are_dropped():
    p = RNG.uniform(0, 10, (1, 3))
    same = np.repeat(p, 3, axis=0)                               # rigid: covariance of rank 0
    line = np.outer(np.arange(4.0), [1.0, 2.0, -1.0]) + 5.0      # affine: four collinear points, design matrix of rank 2
    good_f, good_m, _ = mo.make_pair(3, 8, 5, drop=0.0, n_outliers=0)
    for tt, bad in (("rigid", same), ("affine", line)):
        n = len(bad)
        with pytest.raises(ValueError, match="degenerate"):
            mo.fit_transform(bad, bad + 1.0, tt)
        with pytest.raises(ValueError, match="degenerate"):
            mr.fit_transform(bad, bad + 1.0, tt)
        _, valid = mr.fit_transforms_batch(np.stack([good_f[:n], bad, good_f[1:n + 1]]), np.stack([good_m[:n], bad + 1.0, good_m[1:n + 1]]), tt)
        assert valid.tolist() == [True, False, True]


def _sim(shape=(8, 16, 20), origin=(2.0, -3.0, 10.0), spacing=(2.0, 0.5, 1.0)):
    sim = si.to_spatial_image(np.zeros(shape, np.uint16), dims=["z", "y", "x"], scale=dict(zip("zyx", spacing)),
                              translation=dict(zip("zyx", origin)))
    si.set_sim_affine(sim, np.eye(4), "stage")
    return sim


def test_point_sets_round_trip_and_follow_selections():
    sim = _sim()
    pts = np.array([[4.0, 0.0, 12.0], [np.nan, 1.0, 13.0], [10.0, 2.5, 20.0], [16.0, 4.5, 29.0], [3.0, -3.0, 10.0]])
    msim = msi_utils.get_msim_from_sim(sim, scale_factors=[2])
    with pytest.raises(KeyError, match="'beads'"):
        msi_utils.get_point_set(msim)
    msi_utils.set_point_set(msim, pts)
    msi_utils.set_point_set(msim, pts[:2] + 1.0, points_key="other")
    got = msi_utils.get_point_set(msim, "beads")
    assert got.dtype == np.float64 and np.array_equal(got, pts, equal_nan=True) and got is not pts
    for scale in ("scale0", "scale1"):
        s = msi_utils.get_sim_from_msim(msim, scale=scale)
        assert np.array_equal(si.get_point_set(s, "beads"), pts, equal_nan=True)
        assert np.array_equal(si.get_point_set(s, "other"), pts[:2] + 1.0, equal_nan=True)
    with pytest.raises(ValueError, match="n_points, 3"):
        msi_utils.set_point_set(msim, np.zeros((4, 2)))
    s0 = msi_utils.get_sim_from_msim(msim)
    # the closed interval of a selection: a point exactly on either border stays, NaN rows fail every comparison
    sel = si.sim_sel_coords(s0, {"z": slice(4.0, 10.0), "x": slice(12.0, 20.0)})
    assert np.array_equal(si.get_point_set(sel), pts[[0, 2]])
    assert sel.shape == (4, 16, 9) and np.array_equal(si.get_point_set(s0), pts, equal_nan=True)      # the source keeps its points
    assert len(si.get_point_set(si.sim_sel_coords(s0, {"y": slice(100.0, 200.0)}))) == 0
    # reading for registration: non-finite rows dropped, the view's affine applied
    aff = np.eye(4)
    aff[:3, 3] = [1.0, 2.0, 3.0]
    reg = registration._points_for_registration(s0, "beads", ["z", "y", "x"], aff)
    assert np.array_equal(reg, pts[[0, 2, 3, 4]] + [1.0, 2.0, 3.0])
    assert registration._points_for_registration(s0, "beads", ["z", "y", "x"], aff, {"z": slice(100.0, 101.0)}).shape == (0, 3)


def _two_views(shift=(0.0, 0.0, 0.0)):
    """Two 8 x 16 x 20 views, the second 12 voxels to the right of the first (overlap: x in [22, 29] of the first's frame)."""
    a, b = _sim(), _sim(origin=(2.0, -3.0, 22.0))
    t = np.eye(4)
    t[:3, 3] = shift
    si.set_sim_affine(b, t, "stage")
    return a, b


def test_the_seam_passes_transformed_points_and_keeps_a_point_on_the_prefilter_border():
    a, b = _two_views(shift=(0.5, 0.0, 0.0))
    tol = 1e-6
    # view a's window along x is [22 - tol - 1, 29 + tol + 1] in its own frame: 21 - tol sits exactly on its border
    border = 22.0 - tol - 1.0
    pa = np.array([[4.0, 0.0, border], [4.0, 0.0, np.nextafter(border, -np.inf)], [6.0, 1.0, 25.0], [np.inf, 0.0, 25.0], [6.0, 1.0, 12.0]])
    pb = np.array([[4.0, 0.0, 23.0], [6.0, 1.0, 41.0], [8.0, 2.0, 29.0 + tol + 1.0]])
    si.set_point_set(a, pa, "beads")
    si.set_point_set(b, pb, "beads")
    seen = {}

    def reg_func(fixed_points, moving_points, offset=0.0):
        seen["fixed"], seen["moving"] = fixed_points, moving_points
        m = np.eye(4)
        m[2, 3] = offset
        return {"affine_matrix": m, "quality": 0.5}

    res = registration.register_pair_of_msims(a, b, "stage", pairwise_reg_func=reg_func, pairwise_reg_func_kwargs={"offset": 2.0})
    assert np.array_equal(seen["fixed"], pa[[0, 1, 2, 4]]) and np.array_equal(seen["moving"], pb + [0.5, 0.0, 0.0])
    assert res["transform"][2, 3] == 2.0 and res["quality"] == 0.5 and res["bbox"].shape == (2, 3)     # the physical transform, unchanged
    registration.register_pair_of_msims(a, b, "stage", pairwise_reg_func=reg_func, prefilter_markers=True)
    assert np.array_equal(seen["fixed"], pa[[0, 2]])
    assert np.array_equal(seen["moving"], pb[[0, 2]] + [0.5, 0.0, 0.0])
    # another key, through compute_pairwise_registrations
    si.set_point_set(a, pa[:1], "few")
    si.set_point_set(b, pb[:1], "few")
    out = registration.compute_pairwise_registrations([a, b], [(0, 1)], "stage", pairwise_reg_func=reg_func, points_key="few")
    assert len(seen["fixed"]) == 1 and len(out) == 1
    with pytest.raises(KeyError, match="missing"):
        registration.register_pair_of_msims(a, b, "stage", pairwise_reg_func=reg_func, points_key="missing")


def test_a_function_with_only_fixed_points_is_refused():
    a, b = _two_views()

    def half(fixed_points):
        return {"affine_matrix": np.eye(4), "quality": 1.0}

    with pytest.raises(ValueError) as e:
        registration.register_pair_of_msims(a, b, "stage", pairwise_reg_func=half)
    assert str(e.value) == "Point-aware pairwise registration functions must accept both 'fixed_points' and 'moving_points'."


def test_image_data_goes_only_to_functions_that_take_it():
    a, b = _two_views()
    si.set_point_set(a, np.zeros((1, 3)))
    si.set_point_set(b, np.zeros((1, 3)))
    seen = {}

    def both(fixed_points, moving_points, fixed_data, moving_data):
        seen["shapes"] = (tuple(fixed_data.shape), tuple(moving_data.shape))
        return {"affine_matrix": np.eye(4), "quality": 1.0}

    with warnings.catch_warnings():
        warnings.simplefilter("error")       # the constant check is skipped: all-zero crops do not warn
        registration.register_pair_of_msims(a, b, "stage", pairwise_reg_func=both)
    assert seen["shapes"] == ((8, 16, 9), (8, 16, 9))
