"""GPU: mvs_knn against a brute-force yardstick at the edges of its paths, mvs_marker_descriptors and mvs_marker_score against
numpy, registration.registration_marker_based against the restatement of the reference (tests/marker_oracle.py) -- candidates,
inliers, quality and mapped points -- and end to end through the point-set seam of register()."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import marker_oracle as mo

pytestmark = pytest.mark.gpu

# distances: two float64 summation orders of dim + 1 terms and a root differ by at most (dim + 2) 2^-53 relative, 1.9e-15 at
# dim 15; 1e-13 is 50 times that (a derived bound, not a measurement)
RTOL = 1e-13

N_REF = [1, 5, 255, 256, 257, 513]       # one row, fewer than k, around the tile of 256 reference rows, three tiles
N_QUERY = [1, 257]                       # one thread, two workgroups (the second with a single live thread)
DIMS = [1, 2, 3, 6, 10, 15, 7]           # every compiled dimension, the maximum and the loop
KS = [1, 2, 5, 11, 16]                   # every compiled list length and two values between


@functools.lru_cache(maxsize=None)
def _rows(n, dim, seed):
    a = np.random.default_rng(seed).uniform(0.0, 100.0, (n, dim))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _yardstick(n_ref, n_query, dim, k):
    idx, dist = mo.brute_knn(_rows(n_ref, dim, 100 + dim), _rows(n_query, dim, 200 + dim), k)
    idx.setflags(write=False)
    dist.setflags(write=False)
    return idx, dist


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", DIMS)
def test_knn_matches_the_brute_force_yardstick(hip_device, dim, k):
    from multiview_stitcher_amd import _marker_ops as ops

    for n_ref in N_REF:
        for n_query in N_QUERY:
            want_idx, want_dist = _yardstick(n_ref, n_query, dim, k)
            idx, dist = ops.knn(_rows(n_ref, dim, 100 + dim), _rows(n_query, dim, 200 + dim), k, hip_device)
            assert idx.dtype == np.int32 and dist.dtype == np.float64 and idx.shape == dist.shape == (n_query, k)
            assert np.array_equal(idx, want_idx), (n_ref, n_query)
            np.testing.assert_allclose(dist, want_dist, rtol=RTOL, atol=0.0)
            if k > n_ref:
                assert (idx[:, n_ref:] == -1).all() and np.isposinf(dist[:, n_ref:]).all()


@pytest.mark.parametrize("dim,k", [(3, 6), (6, 5), (15, 16)])
def test_knn_device_resident_sets_give_the_bits_of_host_sets(hip_device, dim, k):
    from multiview_stitcher_amd import _marker_ops as ops

    ref, query = _rows(513, dim, 1), _rows(257, dim, 2)
    want = ops.knn(ref, query, k, hip_device)
    dref, dquery = ops.to_device(ref, hip_device), ops.to_device(query, hip_device)
    for r, q in ((dref, dquery), (dref, query), (ref, dquery)):
        got = ops.knn(r, q, k, hip_device)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    self_host, self_dev = ops.knn(ref, ref, k, hip_device), ops.knn(dref, dref, k, hip_device)      # a set against itself: staged once
    assert np.array_equal(self_host[0], self_dev[0]) and np.array_equal(self_host[1], self_dev[1])
    assert np.array_equal(self_host[0], mo.brute_knn(ref, ref, k)[0])


def test_knn_orders_ties_by_lower_index(hip_device):
    """Points on a coarse integer lattice, many of them exact duplicates: squared distances are small integers, so equal
    distances are equal bits on both sides and the order among them is the index."""
    from multiview_stitcher_amd import _marker_ops as ops

    pts = np.random.default_rng(3).integers(0, 4, (300, 3)).astype(np.float64)
    assert len(np.unique(pts, axis=0)) < 100
    for k in (1, 2, 8, 16):
        idx, dist = ops.knn(pts, pts, k, hip_device)
        want_idx, want_dist = mo.brute_knn(pts, pts, k)
        assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
    assert (ops.knn(pts, pts, 16, hip_device)[0][:, 0] <= np.arange(300)).all()      # the first hit of a duplicate is its first copy


def test_knn_indices_survive_a_shift_by_1e6(hip_device):
    from multiview_stitcher_amd import _marker_ops as ops

    # coordinates on a grid of 2^-10: the shifted differences are exact, so the shifted set must give the same bits
    grid = np.random.default_rng(4).integers(0, 200 * 1024, (400, 3)).astype(np.float64) / 1024.0
    idx, dist = ops.knn(grid, grid, 6, hip_device)
    sidx, sdist = ops.knn(grid + 1e6, grid + 1e6, 6, hip_device)
    assert np.array_equal(idx, sidx) and np.array_equal(dist, sdist)
    # any coordinates: the same indices as the unshifted set (the expanded form |a|^2 + |b|^2 - 2ab keeps no digit at 1e12)
    free = _rows(400, 3, 5)
    assert np.array_equal(ops.knn(free + 1e6, free + 1e6, 6, hip_device)[0], ops.knn(free, free, 6, hip_device)[0])
    assert np.array_equal(ops.knn(free + 1e6, free + 1e6, 6, hip_device)[0], mo.brute_knn(free + 1e6, free + 1e6, 6)[0])


def test_bad_arguments_return_error_codes(hip_device):
    from multiview_stitcher_amd import _lib, _marker_ops as ops

    lib = _lib.init(hip_device)
    a = np.zeros((8, 16))
    idx, dist = np.zeros((8, 17), np.int32), np.zeros((8, 17))
    pi, pd = idx.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(C.POINTER(C.c_double))
    p = C.c_void_p(a.ctypes.data)
    knn = lambda ref=p, rmem=0, nr=8, q=p, qmem=0, nq=8, dim=3, k=2, i=pi, d=pd: lib.mvs_knn(hip_device, ref, rmem, nr, q, qmem, nq, dim, k, i, d)
    assert knn() == 0
    assert knn(dim=16) == -4 and knn(k=17) == -4                    # MVS_ERR_UNSUPPORTED
    assert knn(dim=0) == -1 and knn(k=0) == -1 and knn(nr=0) == -1 and knn(nq=-1) == -1
    assert knn(ref=None) == -1 and knn(q=None) == -1 and knn(i=None) == -1 and knn(d=None) == -1
    assert knn(rmem=2) == -1 and knn(qmem=-1) == -1
    assert b"mvs_knn" in lib.mvs_last_error(hip_device)
    with pytest.raises(NotImplementedError, match="dim"):
        ops.knn(a, a, 2, hip_device)
    with pytest.raises(NotImplementedError, match="k = 17"):
        ops.knn(a[:, :3], a[:, :3], 17, hip_device)
    nbr = np.zeros((8, 4), np.int32)
    out = np.zeros((8 * 4, 6))
    pn, po = nbr.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(out.ctypes.data)
    desc = lambda pts=p, mem=0, n=8, ndim=3, nb=pn, nn=3, red=1, o=po, omem=0: lib.mvs_marker_descriptors(hip_device, pts, mem, n, ndim, nb, nn, red, o, omem)
    assert desc() == 0
    assert desc(ndim=1) == -1 and desc(ndim=4) == -1 and desc(nn=0) == -1 and desc(red=-1) == -1 and desc(n=0) == -1
    assert desc(nn=6) == -4 and desc(red=12) == -4
    assert desc(pts=None) == -1 and desc(nb=None) == -1 and desc(o=None) == -1 and desc(mem=3) == -1 and desc(omem=3) == -1
    aff = np.tile(np.eye(4), (2, 1, 1))
    cnt, sm = np.zeros(2, np.int32), np.zeros(2)
    dp = C.POINTER(C.c_double)
    pa, pf, pc, ps = aff.ctypes.data_as(dp), a.ctypes.data_as(dp), cnt.ctypes.data_as(C.POINTER(C.c_int32)), sm.ctypes.data_as(dp)
    score = lambda A=pa, h=2, f=pf, m=pf, n=8, ndim=3, c=pc, s=ps: lib.mvs_marker_score(hip_device, A, h, f, m, n, ndim, 1.0, c, s)
    assert score() == 0 and cnt.tolist() == [8, 8]
    assert score(ndim=1) == -1 and score(ndim=4) == -1 and score(h=0) == -1 and score(n=0) == -1
    assert score(A=None) == -1 and score(f=None) == -1 and score(m=None) == -1 and score(c=None) == -1 and score(s=None) == -1
    # an out-of-range neighbour index faults nothing: its rows are NaN
    nbr[3, 2] = 99
    nbr[5, 0] = -1
    assert desc(nb=nbr.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    bad_rows = np.isnan(out).all(axis=1).reshape(8, 4)
    assert bad_rows[3].tolist() == [True, False, True, True] and bad_rows[5].tolist() == [True, True, True, False] and not bad_rows[[0, 1, 2, 4, 6, 7]].any()


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("num_neighbors,redundancy", [(1, 0), (2, 1), (3, 1), (3, 2), (5, 1)])
def test_descriptors_match_the_oracle(hip_device, num_neighbors, redundancy, ndim):
    from multiview_stitcher_amd import _marker_ops as ops, _marker_reg as mr

    pts = _rows(300, ndim, 40 + ndim)          # 300 .. 3000 rows: more than one workgroup for every subset count
    want = mo.get_descriptors(pts, num_neighbors, redundancy)
    want_vec = np.array([d["vector"] for d in want])
    want_idx = np.array([d["point_index"] for d in want])
    vec, idx = mr.build_descriptors(ops.to_device(pts, hip_device), num_neighbors, redundancy, hip_device, out_on_device=False)
    assert vec.shape == (300 * math.comb(num_neighbors + redundancy, num_neighbors), math.comb(num_neighbors + 1, 2))
    assert np.array_equal(idx, want_idx)
    np.testing.assert_allclose(vec, want_vec, rtol=RTOL, atol=0.0)
    assert (np.diff(vec, axis=1) >= 0).all()
    on_dev, _ = mr.build_descriptors(pts, num_neighbors, redundancy, hip_device, out_on_device=True)      # host points, device result
    assert np.array_equal(on_dev._buf.download(vec.shape, np.float64), vec)


def _score_numpy(affines, fixed, moving, max_error):
    """Residuals (H, C) in the kernel's evaluation order (rows as ((a0 f0 + a1 f1) + a2 f2) + t), counts and sums by numpy."""
    nd = fixed.shape[1]
    sq = 0.0
    for r in range(nd):
        y = affines[:, r, 0, None] * fixed[None, :, 0]
        for c in range(1, nd):
            y = y + affines[:, r, c, None] * fixed[None, :, c]
        d = (y + affines[:, r, nd, None]) - moving[None, :, r]
        sq = sq + d * d
    res = np.sqrt(sq)
    inl = res <= max_error
    return res, inl.sum(axis=1), np.array([r[m].sum() for r, m in zip(res, inl)])


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("n_corr", [1, 63, 64, 65])
@pytest.mark.parametrize("n_hyp", [1, 64, 1000])
def test_score_matches_numpy_and_repeats_its_bits(hip_device, n_hyp, n_corr, ndim):
    from multiview_stitcher_amd import _marker_ops as ops

    rng = np.random.default_rng(1000 * n_hyp + 10 * n_corr + ndim)
    fixed = rng.uniform(0.0, 50.0, (n_corr, ndim))
    affines = np.tile(np.eye(ndim + 1), (n_hyp, 1, 1))
    affines[:, :ndim, :ndim] += rng.normal(0.0, 0.02, (n_hyp, ndim, ndim))
    affines[:, :ndim, ndim] = rng.normal(0.0, 2.0, (n_hyp, ndim))
    moving = fixed + rng.normal(0.0, 2.0, fixed.shape)
    max_error = 5.0
    res, want_counts, want_sums = _score_numpy(affines, fixed, moving, max_error)
    assert np.abs(res - max_error).min() / max_error > 1e-9, "bad input: a residual sits on the inlier bound"
    assert n_hyp * n_corr < 100 or 0 < want_counts.sum() < n_hyp * n_corr
    counts, sums = ops.score(affines, fixed, moving, max_error, hip_device)
    assert counts.dtype == np.int32 and np.array_equal(counts, want_counts)
    np.testing.assert_allclose(sums, want_sums, rtol=RTOL, atol=0.0)
    again = ops.score(affines, fixed, moving, max_error, hip_device)
    assert np.array_equal(again[0], counts) and np.array_equal(again[1], sums)


# ---- registration_marker_based against the oracle ---------------------------------------------------------------------------------
CASES = {
    "3d": dict(ndim=3, n=200, seed=1),                                                   # 0.15 rad, noise 0.1, 20 % dropped, 20 outliers
    "2d": dict(ndim=2, n=150, seed=2, n_outliers=15),
    "3d-at-1e6": dict(ndim=3, n=257, seed=3, offset=1e6),
    "exact-40": dict(ndim=3, n=40, seed=4, noise=0.0, drop=0.0, n_outliers=0),           # 36 candidates: exhaustive for translation
}


@functools.lru_cache(maxsize=None)
def _scene(case):
    f, m, true = mo.make_pair(**CASES[case])
    for a in (f, m, true):
        a.setflags(write=False)
    return f, m, true


@functools.lru_cache(maxsize=None)
def _oracle(case, transform_type, icp):
    f, m, _ = _scene(case)
    try:
        return mo.registration_marker_based(f, m, transform_type=transform_type, icp=icp)
    except ValueError as e:
        return str(e)


RUNS = [(c, t, False) for c in CASES for t in ("translation", "rigid", "affine")] + [("3d", "rigid", True), ("2d", "affine", True)]


@pytest.mark.parametrize("case,transform_type,icp", RUNS, ids=[f"{c}-{t}{'-icp' if i else ''}" for c, t, i in RUNS])
def test_registration_matches_the_oracle(hip_device, case, transform_type, icp):
    from multiview_stitcher_amd import registration

    f, m, _ = _scene(case)
    want = _oracle(case, transform_type, icp)
    if isinstance(want, str):
        # the model does not apply to the scene (a translation for views rotated by 0.15 rad): the same failure, the same words
        with pytest.raises(ValueError) as e:
            registration.registration_marker_based(f, m, transform_type=transform_type, icp=icp, device=hip_device)
        assert str(e.value) == want
        return
    # a scene that sits on a decision boundary would fail below as "bad input", not as a kernel error
    assert mo.min_margin(want["trace"]) >= 1e-6, want["trace"]
    assert want["trace"]["ransac_key_gap"] >= 1e-6, want["trace"]
    got = registration._marker_registration_details(f, m, transform_type=transform_type, icp=icp, device=hip_device)
    assert np.array_equal(got["candidate_pairs"], want["candidate_pairs"])
    assert np.array_equal(got["inlier_mask"], want["inlier_mask"])
    assert abs(got["quality"] - want["quality"]) <= 1e-12
    scale = np.abs(f).max()
    assert np.abs(mo.transform_pts(f, got["affine_matrix"]) - mo.transform_pts(f, want["affine_matrix"])).max() <= 1e-9 * scale
    res = registration.registration_marker_based(f, m, transform_type=transform_type, icp=icp, device=hip_device)
    assert set(res) == {"affine_matrix", "quality"} and np.array_equal(res["affine_matrix"], got["affine_matrix"]) and res["quality"] == got["quality"]


def test_exhaustive_sampling_is_what_the_exact_case_exercises():
    want = _oracle("exact-40", "translation", False)
    assert math.comb(len(want["candidate_pairs"]), 1) <= 1000 < math.comb(len(want["candidate_pairs"]), 3)


def test_unrelated_sets_fail_or_warn(hip_device):
    from multiview_stitcher_amd import registration

    f, m = _rows(60, 3, 71), _rows(70, 3, 72)
    with pytest.raises(ValueError) as e:
        mo.registration_marker_based(f, m)
    with pytest.raises(ValueError) as e2:
        registration.registration_marker_based(f, m, device=hip_device)
    assert str(e2.value) == str(e.value)
    with pytest.warns(UserWarning) as w:
        res = registration.registration_marker_based(f, m, fail_on_error=False, device=hip_device)
    assert [str(x.message) for x in w] == [str(e.value)]
    assert np.array_equal(res["affine_matrix"], np.eye(4)) and np.isnan(res["quality"])


# ---- through the seam ------------------------------------------------------------------------------------------------------------
SHIFT = np.array([1.5, -2.25, 3.0])
WORLD = (48, 128, 192)
TILE = (48, 128, 128)


def bead_world(seed, n=200):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)) * np.array(WORLD)


def _tile(x0, data=None):
    from multiview_stitcher_amd import msi_utils
    from multiview_stitcher_amd import spatial_image_utils as si

    sim = si.to_spatial_image(np.zeros(TILE, np.uint16) if data is None else data, dims=["z", "y", "x"], scale=dict(zip("zyx", (1.0, 1.0, 1.0))),
                              translation=dict(zip("zyx", (0.0, 0.0, float(x0)))))
    si.set_sim_affine(sim, np.eye(4), "stage")
    return msi_utils.get_msim_from_sim(sim)


def point_views(seed):
    """Two views of one bead field: the first sees x < 124, the second x >= 68; the second view's stage position is off by
    SHIFT (its own coordinates are the world's minus SHIFT), and its detections carry N(0, 0.05) noise."""
    from multiview_stitcher_amd import msi_utils

    world = bead_world(seed)
    rng = np.random.default_rng(seed + 1000)
    p0 = world[world[:, 2] < 124.0]
    p1 = world[world[:, 2] >= 68.0] - SHIFT + rng.normal(0.0, 0.05, (int((world[:, 2] >= 68.0).sum()), 3))
    p1 = p1[rng.permutation(len(p1))]
    m0, m1 = _tile(0), _tile(64)
    msi_utils.set_point_set(m0, p0)
    msi_utils.set_point_set(m1, p1)
    return m0, m1, p0, p1


@functools.lru_cache(maxsize=None)
def _false_inliers_of_the_reference(seed, prefilter):
    """How many inliers of the reference's own result (the oracle's) are not true correspondences in the scene of ``seed``."""
    _, _, p0, p1 = point_views(seed)
    q0, q1 = (_in_window(p) for p in (p0, p1)) if prefilter else (p0, p1)
    want = mo.registration_marker_based(q0, q1, transform_type="translation")
    pairs = want["candidate_pairs"]
    true = np.linalg.norm(q0[pairs[:, 0]] - SHIFT - q1[pairs[:, 1]], axis=1) < 0.5
    return int((want["inlier_mask"] & ~true).sum())


def _in_window(p):
    """The closed windows of the crop selection (lower - 1e-6 - spacing ... upper + 1e-6 + spacing), the same numbers in either
    view's own frame: the overlap is x in [64, 127], all of z and y."""
    lo = np.array([0.0, 0.0, 64.0]) - 1e-6 - 1.0
    hi = np.array([47.0, 127.0, 127.0]) + 1e-6 + 1.0
    return p[np.all((p >= lo) & (p <= hi), axis=1)]


# Seed 2 is left out on the oracle's evidence, not the kernels': there the reference's own best model keeps one FALSE candidate
# within ransac_max_error = 5, which pulls the mean difference of its ~20 inliers by 0.12 -- the 0.1 below presumes true inliers.
@pytest.mark.parametrize("seed", [0, 1, 3])
def test_register_recovers_the_shift_from_point_sets(hip_device, seed):
    from multiview_stitcher_amd import registration

    m0, m1, p0, p1 = point_views(seed)
    for prefilter in (False, True):
        assert _false_inliers_of_the_reference(seed, prefilter) == 0, "bad input: the reference itself keeps a false correspondence"
    for prefilter in (False, True):
        out = registration.register([m0, m1], transform_key="stage", pairwise_reg_func=registration.registration_marker_based,
                                    pairwise_reg_func_kwargs={"transform_type": "translation"},
                                    groupwise_resolution_kwargs={"transform": "translation"}, prefilter_markers=prefilter,
                                    return_dict=True, device=hip_device)
        rel = np.linalg.inv(out["params"][0]) @ out["params"][1]
        # two noise sigma at the few true inliers a rejected model would still need; a missed registration is off by more than 1.5
        assert np.abs(rel[:3, 3] - SHIFT).max() <= 0.1, rel
        assert np.array_equal(rel[:3, :3], np.eye(3))
        pair = out["pairwise_registration"]["results"][0][0]
        q0, q1 = (_in_window(p) for p in (p0, p1)) if prefilter else (p0, p1)
        assert not prefilter or (len(q0) < len(p0) and len(q1) < len(p1))
        direct = registration.registration_marker_based(q0, q1, transform_type="translation", device=hip_device)
        assert np.array_equal(pair["transform"], direct["affine_matrix"]) and pair["quality"] == direct["quality"]
        assert np.abs(pair["transform"][:3, 3] + SHIFT).max() <= 0.1


def render_tile(world, x0, shift_voxels, sigma=1.5):
    """The beads as Gaussian blobs of ``sigma`` in a TILE whose first voxel sits at world x = x0, displaced by ``shift_voxels``."""
    img = np.full(TILE, 100.0)
    r = 6
    g = np.arange(-r, r + 1, dtype=np.float64)
    for p in world - np.array([0.0, 0.0, x0]) - shift_voxels:
        c = np.round(p).astype(int)
        lo, hi = c - r, c + r + 1
        if (hi <= 0).any() or (lo >= np.array(TILE)).any():
            continue
        w = [np.exp(-0.5 * ((ci + g - pi) / sigma) ** 2) for ci, pi in zip(c, p)]
        blob = 3000.0 * w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]
        s_img = tuple(slice(max(l, 0), min(h, n)) for l, h, n in zip(lo, hi, TILE))
        s_blob = tuple(slice(s.start - l, s.stop - l) for s, l in zip(s_img, lo))
        img[s_img] += blob[s_blob]
    return np.clip(np.round(img), 0, 65535).astype(np.uint16)


def test_detect_beads_then_register_recovers_a_voxel_shift(hip_device):
    from multiview_stitcher_amd import detection, msi_utils, registration

    world = bead_world(7)
    shift = np.array([1.0, -2.0, 3.0])
    msims = [_tile(0, render_tile(world, 0, np.zeros(3))), _tile(64, render_tile(world, 64, shift))]
    for m in msims:
        pts = detection.detect_beads(m, detection_func_kwargs={"target_size_physical": 2.0 * np.sqrt(3.0) * 1.5}, device=hip_device)
        assert len(pts) > 60
        msi_utils.set_point_set(m, pts)
    params = registration.register(msims, transform_key="stage", pairwise_reg_func=registration.registration_marker_based,
                                   pairwise_reg_func_kwargs={"transform_type": "translation"},
                                   groupwise_resolution_kwargs={"transform": "translation"}, new_transform_key="registered", device=hip_device)
    rel = np.linalg.inv(params[0]) @ params[1]
    # centroids of integer labels are quantised to half a voxel; the unregistered prior is off by up to three
    assert np.abs(rel[:3, 3] - shift).max() <= 1.0, rel
    assert "registered" in msims[1].transforms
