"""CPU tests of the host algebra of the non-rigid refinement (multiview_stitcher_amd.nonrigid): the block planner, the peak search
with its drop reasons, and the solver -- against known answers and the plain restatement of tests/nonrigid_oracle.py."""
import numpy as np
import pytest

from multiview_stitcher_amd import intensity, nonrigid
from tests import intensity_oracle as io
from tests import metrics_oracle as mo
from tests import nonrigid_cases as nc
from tests import nonrigid_oracle as no


def rotation(ndim, angle):
    m = np.eye(ndim)
    c, s = np.cos(angle), np.sin(angle)
    m[-2:, -2:] = [[c, -s], [s, c]]
    return m


# ---- plan_blocks ----------------------------------------------------------------------------------------------------------------------
PLAN_CASES = {
    "axis-aligned 3D": ((40, 48, 20), 12, (np.eye(3), np.array([0.0, 0.0, 36.0])), (np.eye(3), np.array([0.25, -0.5, 0.4])), (40, 48, 56), (40, 48, 56),
                        (3, 4, 2), (2, 3, 4)),
    "rotated 2D": ((70, 45), (32, 16), (np.eye(2), np.array([3.0, 60.0])), (rotation(2, np.deg2rad(30.0)), np.array([20.3, -27.7])), (96, 120), (96, 120),
                   (4, 5), (3, 3)),
}


@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_blocks_tiles_the_grid_and_takes_the_cells_of_the_box_centres(name):
    grid_shape, block, fa, ma, shape_f, shape_m, nodes_f, nodes_m = PLAN_CASES[name]
    got = nonrigid.plan_blocks(grid_shape, block, fa, ma, shape_f, shape_m, nodes_f, nodes_m)
    ndim = len(grid_shape)
    bl = (block,) * ndim if isinstance(block, int) else block
    assert got.dtype == np.int64 and got.shape[1:] == (4, ndim)
    count = np.zeros(grid_shape, dtype=np.int64)
    for lo, n, _, _ in got:
        assert np.all(n >= 1) and np.all(n <= bl) and np.all(lo % np.asarray(bl) == 0)
        count[tuple(slice(a, a + k) for a, k in zip(lo, n))] += 1
    assert np.all(count == 1)                                           # the boxes tile the grid exactly
    partial = [tuple(n) for _, n, _, _ in got if tuple(n) != tuple(bl)]
    assert partial and all(any(s % b and k == s % b for s, b, k in zip(grid_shape, bl, n)) for n in partial)       # partial boxes are kept
    assert len(got) == int(np.prod([-(-s // b) for s, b in zip(grid_shape, bl)]))
    for lo, n, cf, cm in got:                                           # the cell rule at the clamped pixel coordinate of the centre
        ctr = lo + (n - 1) / 2.0
        for affine, shape, nodes, cell in ((fa, shape_f, nodes_f, cf), (ma, shape_m, nodes_m, cm)):
            pix = np.clip(affine[0] @ ctr + affine[1], 0.0, np.asarray(shape) - 1.0)
            want = [int(np.clip(np.floor((pix[ax] + 0.5) * nodes[ax] / shape[ax]), 0, nodes[ax] - 1)) for ax in range(ndim)]
            assert list(cell) == want
    assert np.array_equal(got, no.plan_blocks(grid_shape, bl, fa, ma, shape_f, shape_m, nodes_f, nodes_m))
    if name == "rotated 2D":
        raw = (got[:, 0] + (got[:, 1] - 1) / 2.0) @ ma[0].T + ma[1]
        assert len({tuple(c) for c in got[:, 3]}) > 1 and np.any(raw < 0)      # a centre outside the tile: clamped


# ---- shifts_from_moments --------------------------------------------------------------------------------------------------------------
def moments_with_ncc(c, n=500.0):
    """Rows of moments whose NCC is ``c`` (NaN: a constant moving block) with ``n`` sample pairs each."""
    c = np.asarray(c, dtype=np.float64)
    m = np.zeros(c.shape + (6,))
    m[..., 0] = n
    m[..., 3] = 4.0
    m[..., 4] = np.where(np.isnan(c), 0.0, 9.0)
    m[..., 5] = np.where(np.isnan(c), 0.0, c * 6.0)
    return m


def parabola(radius, vertex, curvature, top=0.9):
    idx = np.meshgrid(*[np.arange(-r, r + 1, dtype=np.float64) for r in radius], indexing="ij")
    return top - sum(k * (i - v) ** 2 for k, i, v in zip(curvature, idx, vertex))


def test_shifts_from_moments_returns_the_vertex_of_a_parabola():
    radius = (2, 3, 3)
    vertex = (0.3, -1.25, 1.4)
    c = parabola(radius, vertex, (0.02, 0.01, 0.015))
    got = nonrigid.shifts_from_moments(moments_with_ncc(c.reshape(1, -1)), radius, 64, 0.3)
    assert got["reason"] == [None]
    np.testing.assert_allclose(got["shift"][0], vertex, atol=1e-12)     # a separable parabola: the three-point fit is exact
    peak = c.max()
    assert got["weight"][0] == pytest.approx(500.0 * peak) and got["ncc"][0] == pytest.approx(peak)
    want = no.shifts_from_moments(moments_with_ncc(c.reshape(1, -1)), radius, 64, 0.3)[0]
    np.testing.assert_allclose(got["shift"][0], want["shift"], atol=1e-15)
    # 2D: radius 0 along an axis gives shift 0 there, and the clip holds the step at half a pixel
    c2 = parabola((0, 2, 2), (0.0, 0.45, -1.0), (0.0, 0.05, 0.05)).reshape(1, -1)
    got2 = nonrigid.shifts_from_moments(moments_with_ncc(c2), (0, 2, 2), 64, 0.3)
    np.testing.assert_allclose(got2["shift"][0], (0.0, 0.45, -1.0), atol=1e-12)


DROP_CASES = {
    "few_samples": dict(n=63.0),
    "low_ncc": dict(top=0.29),
    "rim": dict(vertex=(0.0, 2.2, 0.0)),
    "flat": dict(flatten=True),
}


@pytest.mark.parametrize("reason", list(DROP_CASES))
def test_shifts_from_moments_drops_with_the_reason(reason):
    case = DROP_CASES[reason]
    radius = (1, 2, 2)
    c = parabola(radius, case.get("vertex", (0.0, 0.2, -0.3)), (0.02, 0.02, 0.02), case.get("top", 0.9))
    if case.get("flatten"):
        k = np.unravel_index(np.argmax(c), c.shape)
        c[k[0], k[1], k[2] + 1] = np.nan                                # a neighbour of the peak that has no NCC
    m = moments_with_ncc(c.reshape(1, -1), case.get("n", 500.0))
    got = nonrigid.shifts_from_moments(m, radius, 64, 0.3)
    assert got["reason"] == [reason] and np.all(np.isnan(got["shift"])) and got["weight"][0] == 0.0
    assert no.shifts_from_moments(m, radius, 64, 0.3)[0]["reason"] == reason
    kept = nonrigid.shifts_from_moments(moments_with_ncc(parabola(radius, (0.0, 0.2, -0.3), (0.02,) * 3).reshape(1, -1)), radius, 64, 0.3)
    assert kept["reason"] == [None]


def test_shifts_from_moments_on_plateaus_and_without_any_ncc():
    """A first maximum in index order has no earlier equal: c- < c0 on every axis, so the second difference of a peak with two
    finite neighbours is negative and ``flat`` comes from NaN neighbours; a plateau's first maximum is its first index, on the rim."""
    radius = (0, 1, 1)
    plateau = np.full((1, 9), 0.5)
    assert nonrigid.shifts_from_moments(moments_with_ncc(plateau), radius, 64, 0.3)["reason"] == ["rim"]
    ridge = np.array([[0.2, 0.2, 0.2, 0.4, 0.8, 0.8, 0.2, 0.2, 0.2]])   # (y, x) = (1, 1) ties with (1, 2): the first is kept, c+ = c0
    got = nonrigid.shifts_from_moments(moments_with_ncc(ridge), radius, 64, 0.3)
    assert got["reason"] == [None]
    np.testing.assert_allclose(got["shift"][0], (0.0, 0.0, 0.5), atol=1e-12)
    nan_all = np.full((2, 9), np.nan)
    assert nonrigid.shifts_from_moments(moments_with_ncc(nan_all), radius, 64, 0.3)["reason"] == ["low_ncc", "low_ncc"]
    assert nonrigid.shifts_from_moments(moments_with_ncc(nan_all, n=0.0), radius, 64, 0.3)["reason"] == ["few_samples"] * 2
    assert [r["reason"] for r in no.shifts_from_moments(moments_with_ncc(nan_all), radius, 64, 0.3)] == ["low_ncc", "low_ncc"]


def test_shifts_from_moments_takes_the_first_of_tied_maxima():
    radius = (0, 2, 2)
    c = parabola(radius, (0.0, 0.0, 0.0), (0.0, 0.05, 0.05)).reshape(5, 5)
    c[2, 2] = c[2, 3] = 0.9                                             # a tie between shift (0, 0) and (0, 1): index order takes (0, 0)
    got = nonrigid.shifts_from_moments(moments_with_ncc(c.reshape(1, -1)), radius, 64, 0.3)
    want = no.shifts_from_moments(moments_with_ncc(c.reshape(1, -1)), radius, 64, 0.3)[0]
    assert got["reason"] == [None] and want["index"] == (0, 2, 2) and want["runner_up"] == want["peak"]
    # c- = 0.85, c0 = 0.9, c+ = 0.9 along x: 0.5 * (0.85 - 0.9) / (0.85 - 1.8 + 0.9) = 0.5
    np.testing.assert_allclose(got["shift"][0], (0.0, 0.0, 0.5), atol=1e-12)
    np.testing.assert_allclose(got["shift"][0], want["shift"], atol=1e-15)


# ---- solve_fields ---------------------------------------------------------------------------------------------------------------------
def synthetic_records(nodes, truth, rng, per_pair=40):
    """Consistent records between the views 0-1, 1-2 and 0-2: s_world = u_M - u_F at random cells, random positive weights."""
    recs = []
    for vf, vm in ((0, 1), (1, 2), (0, 2)):
        for _ in range(per_pair):
            cf = tuple(int(rng.integers(0, g)) for g in nodes[vf])
            cm = tuple(int(rng.integers(0, g)) for g in nodes[vm])
            recs.append((vf, vm, cf, cm, truth[vm][cm] - truth[vf][cf], float(rng.uniform(50, 500))))
    return recs


def smooth_truth(nodes, rng, ndim):
    out = []
    for nv in nodes:
        idx = np.stack(np.meshgrid(*[np.linspace(-1, 1, g) if g > 1 else np.zeros(1) for g in nv], indexing="ij"), axis=-1)
        out.append(idx @ rng.normal(0, 0.5, (ndim, ndim)) + rng.normal(0, 0.3, ndim))
    return out


def test_solve_fields_recovers_known_vectors_up_to_the_gauge():
    rng = np.random.default_rng(3)
    nodes = [(2, 3, 3), (1, 2, 4), (3, 2, 2)]
    truth = smooth_truth(nodes, rng, 3)
    recs = synthetic_records(nodes, truth, rng, per_pair=120)
    eye, one = [np.eye(3)] * 3, [np.ones(3)] * 3
    covered = [np.zeros(nv, bool) for nv in nodes]
    for vf, vm, cf, cm, _, _ in recs:
        covered[vf][cf] = covered[vm][cm] = True
    assert all(c.all() for c in covered)
    got = nonrigid.solve_fields(nodes, recs, eye, one, lambda_identity=1e-9, lambda_smooth=0.0)
    assert all(g.dtype == np.float32 and g.shape == nv + (3,) for g, nv in zip(got, nodes))
    gauge = np.mean(np.concatenate([(g - t).reshape(-1, 3) for g, t in zip(got, truth)]), axis=0)
    for g, t in zip(got, truth):                                        # the data term fixes u up to one vector for all cells
        np.testing.assert_allclose(g - gauge, t, atol=2e-6)
    ref, info = nonrigid.solve_fields(nodes, recs, eye, one, lambda_identity=1e-9, lambda_smooth=0.0, reference_view=1, return_info=True)
    assert np.all(ref[1] == 0)
    assert set(info["pairs"]) == {(0, 1), (1, 2), (0, 2)} and all(p["used"] == 120 for p in info["pairs"].values())
    free = nonrigid.solve_fields(nodes, recs, eye, one, lambda_identity=1e-9, lambda_smooth=0.0, return_info=True)[1]
    assert all(p["rms_after"] < 1e-6 < p["rms_before"] for p in free["pairs"].values())
    with pytest.raises(ValueError, match="lambda_identity"):
        nonrigid.solve_fields(nodes, recs, eye, one, lambda_identity=0.0)
    with pytest.raises(ValueError, match="lambda_identity"):
        nonrigid.solve_fields(nodes, recs, eye, one, lambda_identity=-1.0)


def test_solve_fields_equals_three_scalar_solves_and_the_oracle():
    rng = np.random.default_rng(5)
    nodes = [(2, 2, 3), (2, 3, 2), (1, 2, 2)]
    truth = smooth_truth(nodes, rng, 3)
    recs = [(vf, vm, cf, cm, s + rng.normal(0, 0.05, 3), w) for vf, vm, cf, cm, s, w in synthetic_records(nodes, truth, rng)]
    eye, one = [np.eye(3)] * 3, [np.ones(3)] * 3
    kw = dict(lambda_identity=0.05, lambda_smooth=0.1)
    got = nonrigid.solve_fields(nodes, recs, eye, one, **kw)
    want = no.solve(nodes, recs, **kw)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, atol=1e-6)
    for ax in range(3):                                                 # each axis alone: the other components zeroed
        only = [(vf, vm, cf, cm, s * np.eye(3)[ax], w) for vf, vm, cf, cm, s, w in recs]
        alone = nonrigid.solve_fields(nodes, only, eye, one, **kw)
        for a, g in zip(alone, got):
            assert np.array_equal(a[..., ax], g[..., ax]) and not np.any(np.delete(a, ax, axis=-1))
    # the solution is a minimum of the objective: every perturbation raises it
    base = no.objective(nodes, recs, want, **kw)
    for _ in range(5):
        moved = [w + rng.normal(0, 1e-3, w.shape) for w in want]
        assert no.objective(nodes, recs, moved, **kw) > base
    ref = nonrigid.solve_fields(nodes, recs, eye, one, reference_view=2, **kw)
    assert not ref[2].any() and ref[0].any()
    for g, w in zip(ref, no.solve(nodes, recs, reference_view=2, **kw)):
        np.testing.assert_allclose(g, w, atol=1e-6)


def test_solve_fields_returns_pixels_of_a_rotated_anisotropic_view():
    rng = np.random.default_rng(7)
    nodes = [(1, 2, 2), (2, 2, 2)]
    L = [np.eye(3), rotation(3, np.deg2rad(30.0))]
    spacing = [np.ones(3), np.array([2.0, 1.0, 1.0])]
    recs = []
    for _ in range(60):
        cf, cm = tuple(int(rng.integers(0, g)) for g in nodes[0]), tuple(int(rng.integers(0, g)) for g in nodes[1])
        recs.append((0, 1, cf, cm, rng.normal(0, 1.0, 3), float(rng.uniform(10, 100))))
    kw = dict(lambda_identity=0.05, lambda_smooth=0.1)
    world = nonrigid.solve_fields(nodes, recs, [np.eye(3)] * 2, [np.ones(3)] * 2, **kw)
    got = nonrigid.solve_fields(nodes, recs, L, spacing, **kw)
    want_u = no.solve(nodes, recs, **kw)
    for v in range(2):
        want = (want_u[v].reshape(-1, 3) @ np.linalg.inv(L[v]).T / spacing[v]).reshape(nodes[v] + (3,))
        np.testing.assert_allclose(got[v], want, atol=1e-6)
        np.testing.assert_allclose(world[v], want_u[v], atol=1e-6)
    assert np.abs(got[1] - world[1]).max() > 0.05                       # (the rotation and the spacing do something)
    u1 = world[1].reshape(-1, 3).astype(np.float64)
    np.testing.assert_allclose(got[1].reshape(-1, 3)[:, 0], u1[:, 0] / 2.0, atol=1e-6)      # z is not rotated: only the spacing


def test_solve_fields_dense_and_sparse_routes_agree(monkeypatch):
    rng = np.random.default_rng(9)
    nodes = [(3, 4), (4, 3), (2, 5)]
    truth = smooth_truth(nodes, rng, 2)
    recs = [(vf, vm, cf, cm, s + rng.normal(0, 0.05, 2), w) for vf, vm, cf, cm, s, w in synthetic_records(nodes, truth, rng)]
    eye, one = [np.eye(2)] * 3, [np.ones(2)] * 3
    dense = nonrigid.solve_fields(nodes, recs, eye, one)
    monkeypatch.setattr(intensity, "DENSE_SOLVE_MAX_UNKNOWNS", 4)
    sparse = nonrigid.solve_fields(nodes, recs, eye, one)
    for d, s in zip(dense, sparse):
        np.testing.assert_allclose(d, s, atol=1e-6)
        assert np.abs(d).max() > 0.05
    empty = nonrigid.solve_fields(nodes, [], eye, one)
    assert all(e.shape == nv + (2,) and not e.any() for e, nv in zip(empty, nodes))


def test_warp_oracle_displacement_is_the_multilinear_interpolation_between_cell_centres():
    """The oracle's own field interpolation against scipy's linear interpolation between the cell centres, constant beyond."""
    rng = np.random.default_rng(11)
    shape, nodes = (24, 40, 72), (1, 2, 5)
    field = rng.uniform(-3, 3, nodes + (3,)).astype(np.float32)
    d = no.displacement(shape, field)
    from scipy.interpolate import RegularGridInterpolator

    for ax in range(3):
        pts = [io.centres(g, n) for g, n in zip(nodes, shape)]
        grid = [p if len(p) > 1 else np.array([p[0], p[0] + 1.0]) for p in pts]
        vals = field[..., ax].astype(np.float64)
        for k, p in enumerate(pts):
            if len(p) == 1:
                vals = np.repeat(vals, 2, axis=k)
        f = RegularGridInterpolator(grid, vals, bounds_error=False, fill_value=None)
        idx = np.stack(np.meshgrid(*[np.clip(np.arange(n, dtype=np.float64), p[0], p[-1]) for n, p in zip(shape, pts)], indexing="ij"), axis=-1)
        np.testing.assert_allclose(d[..., ax], f(idx), atol=2e-5)
    zero = no.warp(rng.integers(0, 60000, (5, 6, 7)).astype(np.uint16), np.zeros((1, 1, 1, 3), np.float32))
    assert zero.dtype == np.uint16


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(nc.FIT))
def test_the_oracle_leaves_margins_on_the_end_to_end_cases(name):
    """What tests/test_nonrigid_gpu.py relies on when it asks for the oracle's kept blocks and drop reasons: no peak, threshold or
    parabola of these inputs is close enough to a decision for 1e-9 of NCC noise to flip it; and the correction helps."""
    fields, info = nc.oracle_fit(name)
    kept = nc.assert_margins(info, min_ncc=nc.FIT[name]["min_ncc"])
    reasons = [f["reason"] for _, found in info["per_pair"].values() for f in found]
    assert kept == reasons.count(None)
    if name == "2d_tight":
        assert reasons.count("rim") >= 4 and reasons.count("low_ncc") >= 4
    else:
        assert info["rms_after"] < 0.7 * info["rms_before"] and nc.oracle_ratio(name) < 0.7
    assert all(np.abs(e).max() <= 1.5 for e in nc.mosaic(nc.FIT[name]["ndim"])["distortions"])


@pytest.mark.parametrize("dtype_name", ["u16", "f32"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_a_block_at_radius_zero_is_the_pair_of_its_box_in_both_oracles(ndim, dtype_name):
    """What test_one_block_at_radius_zero_is_pair_moments_of_its_box of tests/test_nonrigid_gpu.py relies on: the restatements of
    mvs_block_match and of mvs_pair_moments agree on the block it takes, within the tolerances it uses."""
    c = nc.match_case(ndim, dtype_name)
    block = nc.largest_block(c["grid_shape"])
    n = tuple(int(v) for v in block[0, 1])
    assert n == ((96, 45) if ndim == 2 else (8, 48, 20)) and int(np.prod(n)) <= 7680
    row = no.block_moments(c["fixed"], c["moving"], c["fixed_affine"], c["moving_affine"], block, (0,) * ndim, c["halfspaces"])[0, 0]
    whole = mo.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], [c["moving_affine"]], n, c["halfspaces"])[0]
    assert row[0] == whole[0] and whole[0] > 500
    np.testing.assert_allclose(row[1:3], whole[1:3], rtol=1e-9)
    np.testing.assert_allclose(row[3:], whole[3:], rtol=1e-9, atol=1e-9 * max(whole[3], whole[4]))
