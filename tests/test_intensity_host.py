"""CPU tests of the tile intensity harmonisation: the cell rule and the tables of the apply kernel, the record planner, the solver
on the oracle's moments, and the argument checks of the two entry points.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, intensity
from tests import intensity_oracle as io
from tests.intensity_helpers import mosaic, pair_case


# ---- cell rule and tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,g", [(52, 3), (52, 1), (52, 52), (40, 2), (5, 5), (13, 16)])
def test_cell_rule_partitions_the_axis(n, g):
    c = np.linspace(-0.5, n - 0.5, 4001)[:-1]
    k = intensity.cell_index(c, g, n)
    assert k.min() == 0 and k.max() == g - 1 and np.all(np.diff(k) >= 0)
    assert np.array_equal(k, io.cell_of(c, g, n))
    ctr = intensity.cell_centres(g, n)
    assert np.array_equal(intensity.cell_index(ctr, g, n), np.arange(g))          # a centre lies in its own cell ...
    assert np.allclose(ctr, (np.arange(g) + 0.5) * n / g - 0.5, rtol=0, atol=1e-12)
    edges = io.cell_edges(g, n)                                                   # ... and the cell changes at k n / g - 0.5
    assert np.array_equal(intensity.cell_index(edges + 1e-9, g, n), np.arange(1, g))
    assert np.array_equal(intensity.cell_index(edges - 1e-9, g, n), np.arange(g - 1))
    assert intensity.cell_index(-3.0, g, n) == 0 and intensity.cell_index(n + 3.0, g, n) == g - 1


@pytest.mark.parametrize("n,g", [(52, 3), (52, 1), (52, 52), (40, 2), (67, 16)])
def test_tables_reproduce_the_multilinear_weights(n, g):
    lower, t = intensity.axis_table(n, g)
    assert lower.dtype == np.int32 and t.dtype == np.float32 and len(lower) == len(t) == n
    if g == 1:
        assert not lower.any() and not t.any()
        return
    assert lower.min() >= 0 and lower.max() <= g - 2 and t.min() >= 0 and t.max() <= 1
    # the float64 weights, derived another way: interpolate the hat function of every cell centre with np.interp (which clamps)
    ctr = intensity.cell_centres(g, n)
    p = np.arange(n, dtype=np.float64)
    for k in range(g):
        hat = np.interp(p, ctr, np.eye(g)[k])
        got = np.where(lower == k, 1.0 - t.astype(np.float64), 0.0) + np.where(lower + 1 == k, t.astype(np.float64), 0.0)
        assert np.abs(got - hat).max() <= 2.0 ** -23, (k, np.abs(got - hat).max())
    lo_o, t_o = io.axis_table(n, g)
    assert np.array_equal(lower, lo_o) and np.array_equal(t, t_o)


# ---- plan_records ------------------------------------------------------------------------------------------------------------------
def labels_of(case):
    ok, _, _, lab_f, lab_m = io.labelled_samples(case["fixed"], case["moving"], case["fixed_affine"], case["moving_affine"], case["grid_shape"],
                                                 case["cells_f"], case["cells_m"], None)
    return ok, lab_f, lab_m


@pytest.mark.parametrize("ndim", [2, 3])
def test_translation_records_tile_the_overlap(ndim):
    shape = (40, 52) if ndim == 2 else (12, 20, 36)
    cells_f, cells_m = ((2, 3), (3, 2)) if ndim == 2 else ((1, 2, 3), (2, 1, 2))
    grid_shape = tuple(s - 3 for s in shape)
    fa = (np.eye(ndim), np.array([3.0, 0.0, 2.0][-ndim:]))
    ma = (np.eye(ndim), np.array([-2.0, 5.0, -7.0][-ndim:]))           # part of the grid lies outside the moving tile
    recs = intensity.plan_records(fa, ma, grid_shape, shape, shape, cells_f, cells_m)
    count = np.zeros(grid_shape, dtype=int)
    cf, cm = io.grid_coords(fa, grid_shape), io.grid_coords(ma, grid_shape)
    for lo, n, kf, km in recs:
        box = tuple(slice(a, a + b) for a, b in zip(lo, n))
        count[box] += 1
        for ax in range(ndim):                                           # exact boxes: every voxel of a box belongs to the record
            assert np.all(io.cell_of(cf[ax][box], cells_f[ax], shape[ax]) == kf[ax])
            assert np.all(io.cell_of(cm[ax][box], cells_m[ax], shape[ax]) == km[ax])
    inside = np.ones(grid_shape, dtype=bool)
    for ax in range(ndim):
        inside &= (cf[ax] >= 0) & (cf[ax] <= shape[ax] - 1) & (cm[ax] >= 0) & (cm[ax] <= shape[ax] - 1)
    assert inside.any() and not inside.all()
    assert np.array_equal(count, inside.astype(int))                     # every in-bounds voxel once, nothing else, no overlap


@pytest.mark.parametrize("ndim,step", [(2, 1), (2, 2), (3, 1)])
def test_rotated_records_are_conservative(ndim, step):
    case = pair_case(ndim, "f32", step)
    recs = intensity.plan_records(case["fixed_affine"], case["moving_affine"], case["grid_shape"], case["fixed"].shape, case["moving"].shape,
                                  case["cells_f"], case["cells_m"])
    ok, lab_f, lab_m = labels_of(case)
    covered = np.zeros(case["grid_shape"], dtype=bool)
    keys = set()
    for lo, n, kf, km in recs:
        assert (tuple(kf), tuple(km)) not in keys
        keys.add((tuple(kf), tuple(km)))
        box = tuple(slice(a, a + b) for a, b in zip(lo, n))
        col = (ndim,) + (1,) * ndim
        mine = np.all(lab_f[(slice(None),) + box] == kf.reshape(col), axis=0) & np.all(lab_m[(slice(None),) + box] == km.reshape(col), axis=0)
        covered[box] |= mine
    assert ok.sum() > 100 and np.all(covered[ok])                        # every counted voxel lies inside the box of its own record


def test_tiles_that_do_not_overlap_give_no_records():
    far = (np.eye(2), np.array([100.0, 0.0]))
    assert len(intensity.plan_records((np.eye(2), np.zeros(2)), far, (40, 52), (40, 52), (40, 52), (2, 3), (3, 2))) == 0
    rot = (np.array([[0.9, -0.1], [0.1, 0.9]]), np.array([0.0, 300.0]))
    assert len(intensity.plan_records((np.eye(2), np.zeros(2)), rot, (40, 52), (40, 52), (40, 52), (2, 3), (3, 2))) == 0


# ---- the solver on oracle moments ---------------------------------------------------------------------------------------------------
def oracle_records(ramp, cells):
    m = mosaic(2, ramp)
    per_view = [cells] * len(m["views"])
    records = []
    for i, j in m["pairs"]:
        g = io.pair_grid(m["views"][i], m["views"][j], "stage")
        mom = io.cell_pair_moments(m["views"][i]["data"], m["views"][j]["data"], g["fixed_affine"], g["moving_affine"], g["grid_shape"], cells, cells,
                                   g["halfspaces"])
        records.extend((i, j, cf, cm, mo) for (cf, cm), mo in mom.items())
    return per_view, records


@pytest.mark.parametrize("kw", [
    {}, {"reference_view": 0}, {"normalize": False}, {"lambda_identity": 1e-3, "lambda_smooth": 0.0, "reference_view": 2},
    {"lambda_smooth": 2.0, "min_samples": 300}])
def test_solver_matches_the_dense_minimiser(kw):
    per_view, records = oracle_records(True, (2, 2))
    got, info = intensity.solve_maps(per_view, records, return_info=True, **kw)
    want, winfo = io.solve(per_view, records, **kw)
    scale = max(np.abs(w).max() for w in want)
    for g, w in zip(got, want):                                          # (float32 on return: 1e-9 plus what the cast costs)
        assert g.dtype == np.float32 and g.shape == w.shape
        assert np.abs(g - w).max() <= 1e-9 * scale + 2.0 ** -24 * scale
    assert abs(info["s"] - winfo["s"]) <= 1e-12 * winfo["s"] and info["N"] == winfo["N"]
    before = sum(p["data_before"] for p in info["pairs"].values())
    after = sum(p["data_after"] for p in info["pairs"].values())
    assert abs(before - winfo["before"]) <= 1e-9 * winfo["before"] and abs(after - winfo["after"]) <= 1e-9 * max(winfo["before"], 1e-300)
    if kw.get("reference_view") is not None:
        ref = got[kw["reference_view"]]
        assert np.all(ref[..., 0] == 1.0) and np.all(ref[..., 1] == 0.0)


def test_solver_float64_solution_matches_to_1e9(monkeypatch):
    """The same comparison before the cast to float32: 1e-9 relative."""
    per_view, records = oracle_records(True, (2, 2))
    captured = {}
    real = np.linalg.solve

    def spy(a, b):
        captured["u"] = real(a, b)
        return captured["u"]

    monkeypatch.setattr(intensity.np.linalg, "solve", spy)
    intensity.solve_maps(per_view, records, normalize=False)
    monkeypatch.undo()
    want, winfo = io.solve(per_view, records, normalize=False)
    u = captured["u"].reshape(-1, 2)
    w = np.concatenate([m.reshape(-1, 2) for m in want])
    w[:, 1] /= winfo["s"]
    assert np.abs(u - w).max() <= 1e-9 * np.abs(w).max()


def test_solver_refuses_a_non_positive_identity_weight():
    per_view, records = oracle_records(False, (1, 1))
    for lam in (0.0, -1.0):
        with pytest.raises(ValueError):
            intensity.solve_maps(per_view, records, lambda_identity=lam)
    with pytest.raises(ValueError):
        intensity.fit_maps([], "stage", lambda_identity=0.0)


@pytest.mark.parametrize("cells,ramp", [((1, 1), False), ((2, 2), True)])
def test_the_solution_does_not_raise_the_data_term(cells, ramp):
    """The identity is feasible at zero penalty, so the objective at the solution is at most the data term at the identity."""
    per_view, records = oracle_records(ramp, cells)
    _, info = intensity.solve_maps(per_view, records, normalize=False, return_info=True)
    before = sum(p["data_before"] for p in info["pairs"].values())
    after = sum(p["data_after"] for p in info["pairs"].values())
    assert set(info["pairs"]) == set(mosaic(2, ramp)["pairs"])
    assert 0 <= after <= before and after < 0.5 * before


def test_a_view_without_usable_records_keeps_the_identity():
    per_view, records = oracle_records(False, (1, 1))
    kept = [r for r in records if 3 not in r[:2]]                        # view 3 loses all its pairs ...
    weak = [(2, 3, (0, 0), (0, 0), np.array([5.0, 1.0, 2.0, 1.0, 1.0, 0.5]))]       # ... but for one record below min_samples
    maps, info = intensity.solve_maps(per_view + [(2, 2)], kept + weak, normalize=False, return_info=True)
    assert np.abs(maps[3] - [1.0, 0.0]).max() <= 1e-6 and np.abs(maps[4] - [1.0, 0.0]).max() <= 1e-6
    assert info["skipped"] == [(2, 3, (0, 0), (0, 0), 5.0)]
    assert np.abs(maps[1][..., 0] - 1.0).max() > 0.01
    none, _ = intensity.solve_maps(per_view, [], return_info=True)
    assert all(np.array_equal(m, np.broadcast_to(np.float32([1, 0]), m.shape)) for m in none)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    assert C.sizeof(_lib.mvs_intensity_record_t) == 72
    data = np.zeros((1, 8, 8), np.float32)
    out = np.zeros(6)

    def view(arr, dtype=_lib.MVS_F32):
        v = _lib.mvs_view_t()
        v.data, v.dtype, v.mem = arr.ctypes.data, dtype, _lib.MVS_MEM_HOST
        v.shape[:] = list(arr.shape)
        v.stride[:] = [arr.shape[1] * arr.shape[2], arr.shape[2], 1]
        return v

    i3 = lambda *v: (C.c_int32 * 3)(*v)
    rec = (_lib.mvs_intensity_record_t * 1)()
    rec[0].n[:] = [1, 4, 4]
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    f, m = view(data), view(data)
    moments = lambda **k: lib.mvs_intensity_pair_moments(0, k.get("f", C.byref(f)), C.byref(k.get("m", m)), k.get("ndim", 2), k.get("cf", i3(1, 2, 2)),
                                                         i3(1, 2, 2), None, k.get("nhs", 0), k.get("rec", rec), k.get("nrec", 1), dp)
    assert moments(f=None) == -1                                         # MVS_ERR_INVALID_ARG
    assert moments(ndim=4) == -1
    assert moments(cf=i3(1, 2, _lib.MVS_INTENSITY_MAX_CELLS + 1)) == -1
    assert moments(cf=i3(2, 2, 2)) == -1                                 # 2D: one cell along z
    assert moments(m=view(data, _lib.MVS_U16)) == _lib.ERR_UNSUPPORTED   # mixed dtypes
    assert moments(nrec=0) == -1 and moments(nrec=_lib.MVS_INTENSITY_MAX_RECORDS + 1) == -1
    assert moments(nhs=3) == -1                                          # halfspaces announced, none given
    bad = (_lib.mvs_intensity_record_t * 1)()
    bad[0].n[:] = [1, 4, 4]
    bad[0].cell_f[:] = [0, 2, 0]
    assert moments(rec=bad) == -1                                        # a cell index outside the grid of cells
    bad[0].cell_f[:] = [0, 0, 0]
    bad[0].n[:] = [1, 0, 4]
    assert moments(rec=bad) == -1                                        # an empty box
    assert lib.mvs_last_error(0)

    coeff = np.ones((1, 2, 2, 2), np.float32)
    tables = np.zeros(8 * 17, np.uint8)
    res = np.zeros((1, 8, 8), np.float32)
    fp = coeff.ctypes.data_as(C.POINTER(C.c_float))
    apply = lambda **k: lib.mvs_intensity_apply(0, k.get("v", C.byref(f)), k.get("ndim", 2), k.get("cells", i3(1, 2, 2)), k.get("coeff", fp),
                                                tables.ctypes.data, k.get("out", res.ctypes.data), k.get("odt", _lib.MVS_F32), k.get("omem", _lib.MVS_MEM_HOST))
    assert apply(v=None) == -1 and apply(coeff=None) == -1 and apply(out=None) == -1
    assert apply(ndim=4) == -1
    assert apply(cells=i3(1, 17, 2)) == -1 and apply(cells=i3(1, 0, 2)) == -1
    assert apply(odt=_lib.MVS_U8) == _lib.ERR_UNSUPPORTED                # neither the input's dtype nor float32
    assert apply(omem=7) == -1
    u16 = view(np.zeros((1, 8, 8), np.uint16), _lib.MVS_U16)
    u16.dtype = 9
    assert apply(v=C.byref(u16)) == _lib.ERR_UNSUPPORTED
