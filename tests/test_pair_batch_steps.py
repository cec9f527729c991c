"""CPU tests of the steps of the batched pair path (registration._register_pairs_batched) and of the driver itself with the one
GPU step (_run_pair_jobs) replaced by a recording stand-in.  The tiles are DeviceArrays with invented, distinct pointers: nothing
here dereferences them.  The plans and the stacked post-processing are tested in tests/test_pair_batch.py."""
import threading
import warnings

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _reg_ops, msi_utils, registration
from multiview_stitcher_amd import spatial_image_utils as si
from multiview_stitcher_amd.device import DeviceArray, _Pending

KEY = "k"


def _fake_tile(index, shape, dtype=np.uint16, pad=None, ticket=0, device=0, last_stride=1):
    """A DeviceArray of ``shape`` at an invented address; ``pad``: per axis, how much larger the allocation it is a window of is."""
    alloc = [int(s) + int(p) for s, p in zip(shape, pad if pad is not None else [0] * len(shape))]
    strides = [int(np.prod(alloc[i + 1:])) * last_stride for i in range(len(alloc))]
    ptr = 0x7F0000000000 + index * 0x100000 + (0 if pad is None else 64 * (index + 1))
    return DeviceArray(None, ptr, shape, strides, dtype, device, pending=_Pending(ticket, None) if ticket else None)


def _sim(data, spacing, origin, t):
    nd = len(spacing)
    sd = "zyx"[-nd:]
    s = si.to_spatial_image(data, dims=list(sd), scale=dict(zip(sd, spacing)), translation=dict(zip(sd, origin)))
    a = np.eye(nd + 1)
    a[:nd, nd] = t
    si.set_sim_affine(s, a, KEY)
    return s


def _mosaic(rng, ndim, n_views, dtype=np.uint16, whole_pixels=False, pad=False, tickets=None):
    """Views of one shape and spacing on the corners of a half-tile grid (every pair overlaps), at non-dyadic positions with a
    sub-pixel jitter -- or, ``whole_pixels``, 12 samples per axis at multiples of 6 samples, so that grids binned by 1, 2 or 3
    coincide."""
    shape = [12] * ndim if whole_pixels else [int(v) for v in rng.integers(6, 13, ndim)]
    spacing = rng.choice([1.0, 0.3, 0.6931, 2.5], ndim)
    origin = rng.normal(0, 50, ndim)
    corners = [np.array(c) for c in np.ndindex(*([2] * ndim))]
    sims = []
    for k in range(n_views):
        c = corners[k % len(corners)] if k else np.zeros(ndim)
        t = c * 6 * spacing if whole_pixels else c * 0.5 * np.array(shape) * spacing + (rng.normal(0, 0.3, ndim) * spacing if k else 0.0)
        data = _fake_tile(k, shape, dtype, rng.integers(1, 5, ndim) if pad else None, 0 if tickets is None else tickets[k])
        sims.append(_sim(data, spacing, origin, t))
    return sims


def _all_pairs(n_views):
    return [(a, b) for a in range(n_views) for b in range(a + 1, n_views)]


# ---- binned coordinates ---------------------------------------------------------------------------------------------------------
def test_binned_coordinates_equal_the_mean_of_every_group_bit_for_bit():
    rng = np.random.default_rng(0)
    n_cases = 0
    for length in list(range(3, 71, 4)) + [70]:
        for b in (1, 2, 3, 4):
            if length // b < 1:
                continue
            views = []
            for _ in range(4):
                o, s = rng.normal(0, 300), rng.choice([0.3, 0.6931, 1.0, 2.5, 1e-3 * (1 + rng.random())])
                views.append(o + s * np.arange(length))
            m = length // b
            want = [c[: m * b].reshape(m, b).mean(axis=1) for c in views]
            for c, w in zip(views, want):
                got = registration._binned_coords(c, b)
                assert got.dtype == np.float64 and got.shape == (m,) and got.tobytes() == w.tobytes()
            got = registration._binned_coords(np.stack(views), b)
            assert got.shape == (4, m) and got.tobytes() == np.stack(want).tobytes()
            n_cases += 1
    assert n_cases >= 70


@pytest.mark.parametrize("same_shape", [True, False])
def test_geometry_of_the_binned_views_is_the_coarsened_coordinates(same_shape):
    rng = np.random.default_rng(1)
    sims = _mosaic(rng, 3, 4)
    if not same_shape:
        sims[2] = _sim(_fake_tile(2, (7, 11, 9)), [0.3, 1.0, 2.5], [1.1, -2.3, 0.7], [0.0, 0.4, 0.0])
    bins = [1, 2, 3]
    geoms, geoms_b = registration._pair_geometry(sims, KEY, bins)
    for s, g, gb in zip(sims, geoms, geoms_b):
        assert g.sim is s and gb.sim is s and gb.t == g.t
        for k, (d, b) in enumerate(zip("zyx", bins)):
            c = np.asarray(s.coords[d], dtype=np.float64)
            m = len(c) // b
            want = c[: m * b].reshape(m, b).mean(axis=1)
            assert gb.coords[k].tobytes() == want.tobytes() and gb.coords[k].flags.c_contiguous and gb.coords[k].dtype == np.float64
            assert gb.shape[k] == m and gb.origin[k] == want[0] and gb.spacing[k] == want[1] - want[0]
    same, same_b = registration._pair_geometry(sims, KEY, [1, 1, 1])
    assert same_b is same      # no binning: one geometry


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def _covered(ndim=2):
    sims = _mosaic(np.random.default_rng(2), ndim, 3)
    return {"sims": sims, "edges": [(0, 1), (1, 2)], "binning": {d: 1 for d in "zyx"[-ndim:]}, "device": 0}


def _replace_data(case, v, **kw):
    old = case["sims"][v]
    shape = kw.pop("shape", old.data.shape)
    case["sims"][v] = _sim(_fake_tile(v, shape, **kw), si.get_spacing_from_sim(old, asarray=True), si.get_origin_from_sim(old, asarray=True),
                           old.attrs["transforms"][KEY][:-1, -1])


def _decline_multiscale(c):
    c["sims"][2] = msi_utils.MultiscaleSpatialImage([c["sims"][2]], dict(c["sims"][2].attrs["transforms"]))


def _decline_host_array(c):
    c["sims"][1].data = np.zeros(c["sims"][1].data.shape, np.uint16)


def _decline_mixed_dtype(c):
    _replace_data(c, 1, dtype=np.uint8)


def _decline_unsupported_dtype(c):
    for v in range(3):
        _replace_data(c, v, dtype=np.int32)


def _decline_non_spatial_dims(c):
    old = c["sims"][1]
    s = si.to_spatial_image(_fake_tile(1, (1,) + old.data.shape), dims=["c", "y", "x"], scale=si.get_spacing_from_sim(old),
                            translation=si.get_origin_from_sim(old))
    si.set_sim_affine(s, old.attrs["transforms"][KEY], KEY)
    c["sims"][1] = s


def _decline_other_device(c):
    _replace_data(c, 2, device=1)


def _decline_last_stride(c):
    _replace_data(c, 0, last_stride=2)


def _decline_rotation(c):
    a = c["sims"][1].attrs["transforms"][KEY].copy()
    a[0, 1], a[1, 0] = 1e-3, -1e-3
    si.set_sim_affine(c["sims"][1], a, KEY)


def _decline_scaling(c):
    a = c["sims"][1].attrs["transforms"][KEY].copy()
    a[0, 0] = 1.0 + 1e-9
    si.set_sim_affine(c["sims"][1], a, KEY)


def _decline_negative_zero(c):
    a = c["sims"][1].attrs["transforms"][KEY].copy()
    a[0, 1] = -0.0
    si.set_sim_affine(c["sims"][1], a, KEY)


def _decline_shapes_differ_without_binning(c):
    _replace_data(c, 2, shape=tuple(s + 1 for s in c["sims"][2].data.shape))
    c["binning"] = None


def _decline_spacings_differ_without_binning(c):
    old = c["sims"][2]
    c["sims"][2] = _sim(old.data, si.get_spacing_from_sim(old, asarray=True) * 1.25, si.get_origin_from_sim(old, asarray=True),
                        old.attrs["transforms"][KEY][:-1, -1])
    c["binning"] = None


def _decline_binned_axis_empty(c):
    c["binning"] = {"y": 1, "x": 13}


# every reason the batched path declines for (the issue's list; "mixed or unsupported dtype", "not a pure translation" and "shapes or
# spacings differ" have one case per alternative)
REASONS = ("multiscale", "host_array", "mixed_dtype", "unsupported_dtype", "non_spatial_dims", "other_device", "last_stride", "rotation",
           "scaling", "negative_zero", "shapes_differ_without_binning", "spacings_differ_without_binning", "binned_axis_empty")


def _coverage(c):
    return registration._batch_coverage(c["sims"], c["edges"], KEY, c["binning"], None, c["device"])


def test_every_reason_to_decline_has_a_case():
    cases = {name[len("_decline_"):] for name in globals() if name.startswith("_decline_")}
    assert cases == set(REASONS)


@pytest.mark.parametrize("reason", REASONS)
def test_coverage_declines(reason):
    c = _covered()
    assert _coverage(c) is not None
    globals()["_decline_" + reason](c)
    assert _coverage(c) is None
    # ... and so does the driver, before it plans or runs anything
    assert registration._register_pairs_batched(c["sims"], c["edges"], KEY, c["binning"], None, None, c["device"], 4, registration._BinCache()) is None


@pytest.mark.parametrize("ndim", [2, 3])
def test_coverage_of_a_minimal_case(ndim):
    c = _covered(ndim)
    b = _coverage(c)
    assert b.used == [0, 1, 2] and b.n == ndim and b.sdims == list("zyx"[-ndim:]) and b.dtype == np.uint16
    assert b.pairs.dtype == np.int32 and b.pairs.tolist() == [[0, 1], [1, 2]]
    assert b.bins == [1] * ndim and not b.do_bin and b.tol == [0.0] * ndim and b.geoms_b is b.geoms
    assert [g.sim for g in b.geoms] == c["sims"]
    # pairs index the USED views; tolerances as a number and as a dict that leaves dims out
    b = registration._batch_coverage(c["sims"], [(2, 0)], KEY, {"x": 2}, 1.5, 0)
    assert b.used == [0, 2] and b.pairs.tolist() == [[1, 0]] and b.tol == [1.5] * ndim and b.bins == [1] * (ndim - 1) + [2] and b.do_bin
    assert registration._batch_coverage(c["sims"], [(2, 0)], KEY, {"x": 2}, {"x": 0.5}, 0).tol == [0.0] * (ndim - 1) + [0.5]
    assert registration._batch_coverage(c["sims"], [], KEY, None, None, 0) is None
    # without a binning: the optimal one of the (equal) views
    assert registration._batch_coverage(c["sims"], c["edges"], KEY, None, None, 0).bins == [1] * ndim


def test_tolerance_and_upsample_defaults():
    assert registration._normalise_tolerance(None, ["y", "x"]) == {"y": 0.0, "x": 0.0}
    assert registration._normalise_tolerance(2, ["y", "x"]) == {"y": 2.0, "x": 2.0}
    assert registration._normalise_tolerance({"x": 1, "z": 3}, ["y", "x"]) == {"y": 0.0, "x": 1.0}
    assert registration._default_upsample_factor(2) == 10 and registration._default_upsample_factor(3) == 2


# ---- crop sources and jobs ------------------------------------------------------------------------------------------------------
def test_crops_come_from_the_raw_tiles_only_for_whole_pixel_integer_mosaics(monkeypatch):
    rng = np.random.default_rng(3)
    for ndim in (2, 3):
        bins = [1, 2, 3][-ndim:]
        plans = {}
        sims = _mosaic(rng, ndim, 4, whole_pixels=True)
        for whole in (True, False):
            if not whole:       # one view a quarter of a sample off the common grid
                off = sims[1].attrs["transforms"][KEY].copy()
                off[ndim - 1, ndim] += 0.25 * si.get_spacing_from_sim(sims[1])["x"]
                si.set_sim_affine(sims[1], off, KEY)
            geoms_b = registration._pair_geometry(sims, KEY, bins)[1]
            plans[whole] = registration._plan_pairs(geoms_b, _all_pairs(4), [0.0] * ndim)
            assert np.all(plans[whole].status == 0)
        u16, u8, f32 = np.dtype(np.uint16), np.dtype(np.uint8), np.dtype(np.float32)
        assert registration._crops_from_raw_tiles(u16, True, plans[True], ndim) is True
        assert registration._crops_from_raw_tiles(u8, True, plans[True], ndim) is True
        assert registration._crops_from_raw_tiles(f32, True, plans[True], ndim) is False          # a float mean is not the truncating cast
        assert registration._crops_from_raw_tiles(u16, False, plans[True], ndim) is False         # nothing to bin
        assert registration._crops_from_raw_tiles(u16, True, plans[False], ndim) is False         # the crops interpolate
        monkeypatch.setattr(registration, "_raw_crops_enabled", [False])
        assert registration._crops_from_raw_tiles(u16, True, plans[True], ndim) is False
        monkeypatch.setattr(registration, "_raw_crops_enabled", [True])


def _expected_job(plans, p, pair, ndim, tiles, tickets, bin_scale, timed):
    """One pair's job, field by field, in plain Python."""
    k0 = 3 - ndim
    scale = bin_scale if bin_scale is not None else [1] * ndim
    want = {"out_shape": [1] * k0 + [int(v) for v in plans.out_shape[p, :ndim]], "bin": [1] * k0 + list(scale) if bin_scale is not None else [0, 0, 0],
            "wait_ticket": [tickets[v] for v in pair], "flags": 1 if timed else 0, "views": []}
    for i, v in enumerate(pair):
        tile = tiles[v]
        start = [int(plans.windows[p, i, k, 0]) * scale[k] for k in range(ndim)]
        stop = [int(plans.windows[p, i, k, 1]) * scale[k] for k in range(ndim)]
        size = [b - a for a, b in zip(start, stop)]
        matrix = [0.0] * 9
        for k in range(3):
            matrix[4 * k] = 1.0 if k < k0 else float(plans.matrix_diag[p, i, k - k0])
        want["views"].append({
            "data": tile.ptr + sum(a * st for a, st in zip(start, tile.strides)) * tile.dtype.itemsize,
            "dtype": _lib.DTYPE_CODES[tile.dtype], "mem": _lib.MVS_MEM_DEVICE, "shape": [1] * k0 + size,
            "stride": list(tile.strides) if ndim == 3 else [tile.strides[0] * size[0]] + list(tile.strides),     # a 2D slab is one z plane
            "matrix": matrix, "offset": [0.0] * k0 + [float(v) for v in plans.offset[p, i, :ndim]]})
    return want


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("binned", [False, True])
def test_jobs_equal_a_per_pair_spelling_field_by_field(ndim, dtype, binned):
    rng = np.random.default_rng(7 * ndim + binned)
    n_views = 5
    tickets = [3, 11, 7, 5, 23]
    sims = _mosaic(rng, ndim, n_views, dtype=dtype, whole_pixels=binned, pad=True, tickets=tickets)
    tiles = [s.data for s in sims]
    assert len({t.ptr for t in tiles}) == n_views and all(t.strides[0] > int(np.prod(t.shape[1:])) for t in tiles)     # windows of larger allocations
    bins = [1, 2, 3][-ndim:] if binned else [1] * ndim
    pairs = np.array(_all_pairs(n_views) + [(3, 1)], dtype=np.int32)
    plans = registration._plan_pairs(registration._pair_geometry(sims, KEY, bins)[1], pairs, [0.0] * ndim)
    assert np.all(plans.status == 0)
    for timed in (False, True):
        jobs = registration._fill_pair_jobs(plans, pairs, ndim, [t.ptr for t in tiles], [t.strides for t in tiles], np.dtype(dtype).itemsize,
                                            _lib.DTYPE_CODES[np.dtype(dtype)], tickets, bins if binned else None, timed)
        assert len(jobs) == len(pairs)
        for p, pair in enumerate(pairs.tolist()):
            want = _expected_job(plans, p, pair, ndim, tiles, tickets, bins if binned else None, timed)
            job = jobs[p]
            for view, w in zip((job.fixed, job.moving), want["views"]):
                assert view.data == w["data"] and view.dtype == w["dtype"] and view.mem == w["mem"]
                assert list(view.shape) == w["shape"] and list(view.stride) == w["stride"]
                assert list(view.matrix) == w["matrix"] and list(view.offset) == w["offset"]
                assert all(s >= 1 for s in w["shape"])
            assert list(job.out_shape) == want["out_shape"] and list(job.bin) == want["bin"]
            assert list(job.wait_ticket) == want["wait_ticket"] and job.flags == want["flags"]


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def _answer(p0, p1, n):
    """What the stand-ins report for the pair of crops at addresses p0, p1: shift, quality, status (some constant overlaps)."""
    h = (p0 // 2 * 7 + p1 // 2 * 13) % 1009
    return [(((h >> k) % 9) - 4) * 0.5 for k in range(n)], 0.05 + (h % 90) / 100.0, 2 if h % 4 == 0 else 0


class _RunRecorder:
    """In the seat of registration._run_pair_jobs."""

    def __init__(self, error=None):
        self.calls, self.error = [], error

    def __call__(self, jobs, edges, n, upsample_factor, n_lanes, device, prebin_lane=None):
        ja = np.frombuffer(jobs, dtype=registration._JOB_DTYPE)
        ptrs = [(int(a), int(b)) for a, b in zip(ja["fixed"]["data"], ja["moving"]["data"])]
        self.calls.append({"ptrs": ptrs, "edges": [tuple(e) for e in edges], "tickets": ja["wait_ticket"].tolist(), "bin": ja["bin"].tolist(),
                           "upsample_factor": upsample_factor, "n_lanes": n_lanes, "device": device, "prebin_lane": prebin_lane})
        if self.error is not None:
            raise self.error
        ans = [_answer(a, b, n) for a, b in ptrs]
        return np.array([a[0] for a in ans], dtype=np.float64).reshape(len(ptrs), n), np.array([a[1] for a in ans]), np.array([a[2] for a in ans], dtype=np.int32)


def _fake_register_views(im0, md0, off0, im1, md1, off1, out_shape, uf, region_mode=None, constant_check=False, device=0):
    t, q, status = _answer(im0.ptr, im1.ptr, len(out_shape))
    return np.array(t, dtype=np.float64), q, status, 5


def _no_register_crops(*a, **k):
    raise AssertionError("device-resident slabs go through register_views")


@pytest.fixture
def stand_ins(monkeypatch):
    run = _RunRecorder()
    monkeypatch.setattr(registration, "_run_pair_jobs", run)
    monkeypatch.setattr(_reg_ops, "register_views", _fake_register_views)
    monkeypatch.setattr(_reg_ops, "register_crops", _no_register_crops)
    monkeypatch.setattr(registration, "_KNIFE_MEMO", {})
    monkeypatch.setattr(registration, "_reference_crop_differs", lambda g1, g2, tol, shape: False)
    return run


def _batched(sims, edges, binning, tol=None, kwargs=None, cache=None, n_lanes=4):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return registration._register_pairs_batched(sims, edges, KEY, binning, tol, kwargs, 0, n_lanes, cache if cache is not None else registration._BinCache())


def _lean(sims, edges, tol):
    geoms = [registration._TileGeom(s, KEY) for s in sims]
    sdims = geoms[0].sdims
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return [registration._lean_register_pair(geoms[i], geoms[j], geoms[i], geoms[j], sdims, tol, None, KEY, 0) for i, j in edges]


def _assert_same_results(got, want):
    assert len(got) == len(want)
    n_const = 0
    for g, w in zip(got, want):
        assert set(g) == set(w) == {"transform", "quality", "bbox"}
        assert g["transform"].tobytes() == w["transform"].tobytes() and g["bbox"].tobytes() == w["bbox"].tobytes()
        assert g["quality"] == w["quality"] or (np.isnan(g["quality"]) and np.isnan(w["quality"]))
        n_const += int(np.isnan(g["quality"]))
    return n_const


def test_driver_results_equal_the_per_pair_path(stand_ins):
    rng = np.random.default_rng(11)
    n_checked = n_const = 0
    for trial in range(6):
        ndim = 2 + trial % 2
        sims = _mosaic(rng, ndim, 5 if trial < 4 else 3, dtype=[np.uint16, np.uint8][trial % 2], pad=trial % 3 == 0)
        edges = _all_pairs(len(sims)) + [(2, 0)]
        tol = [None, 1.5, {"x": 0.5}][trial % 3]
        binning = {d: 1 for d in "zyx"[-ndim:]}
        got = _batched(sims, edges, binning, tol, {"upsample_factor": 4} if trial == 1 else None, n_lanes=3)
        tol_l = list(registration._normalise_tolerance(tol, "zyx"[-ndim:]).values())
        n_const += _assert_same_results(got, _lean(sims, edges, tol_l))
        n_checked += len(edges)
        call = stand_ins.calls[-1]
        assert call["edges"] == edges and call["n_lanes"] == 3 and call["device"] == 0 and call["prebin_lane"] is None
        assert call["upsample_factor"] == (4 if trial == 1 else 10 if ndim == 2 else 2)
        assert call["bin"] == [[0, 0, 0]] * len(edges) and call["tickets"] == [[0, 0]] * len(edges)
    assert len(stand_ins.calls) == 6 and n_checked >= 40 and 1 <= n_const < n_checked


def test_driver_runs_pairs_in_upload_order_and_answers_in_edge_order(stand_ins):
    rng = np.random.default_rng(12)
    tickets = [0, 31, 0, 17, 29]           # three tiles still on their way
    sims = _mosaic(rng, 3, 5, tickets=tickets)
    edges = [(3, 4), (0, 1), (2, 4), (0, 2), (1, 3), (1, 2)]
    order = registration._upload_order(sims, edges)
    assert order == [1, 3, 5, 4, 0, 2]      # by the later tile, ties in the given order
    assert registration._upload_order(sims, [edges[k] for k in order]) is None
    assert registration._upload_order(_mosaic(rng, 3, 5), edges) is None      # nothing in flight: as given
    got = _batched(sims, edges, {"z": 1, "y": 1, "x": 1})
    assert len(stand_ins.calls) == 1
    call = stand_ins.calls[0]
    assert call["edges"] == [edges[k] for k in order]
    assert call["tickets"] == [[tickets[i], tickets[j]] for i, j in call["edges"]]
    _assert_same_results(got, _lean(sims, edges, [0.0] * 3))


def _knife_setup(monkeypatch, rng, ndim, named):
    """A whole-pixel mosaic binned by (1,) 2, 3 (crops from the raw tiles), a crop-length answer that names the pairs ``named`` and
    a recording stand-in for the reference's sequence."""
    sims = _mosaic(rng, ndim, 5, whole_pixels=True)
    edges = _all_pairs(5)
    odd = {(id(sims[i]), id(sims[j])) for i, j in named}
    monkeypatch.setattr(registration, "_reference_crop_differs", lambda g1, g2, tol, shape: (id(g1.sim), id(g2.sim)) in odd)
    redone = []

    def fake_pair(sim1, sim2, transform_key, **kw):
        redone.append((sim1, sim2, transform_key, kw))
        return {"transform": "reference", "quality": len(redone), "bbox": None}

    monkeypatch.setattr(registration, "register_pair_of_msims", fake_pair)
    return sims, edges, redone


@pytest.mark.parametrize("ndim", [2, 3])
def test_driver_sends_knife_edge_pairs_through_the_reference_sequence(monkeypatch, stand_ins, ndim):
    rng = np.random.default_rng(13 + ndim)
    named = [(0, 3), (2, 4), (1, 2)]
    sims, edges, redone = _knife_setup(monkeypatch, rng, ndim, named)
    binning = dict(zip("zyx"[-ndim:], [1, 2, 3][-ndim:]))
    odd = sorted(edges.index(e) for e in named)
    keep = [e for e in range(len(edges)) if e not in odd]
    kwargs = {"upsample_factor": 3}

    def check_redone(cache):
        assert [(a, b) for a, b, _, _ in redone] == [(sims[edges[e][0]], sims[edges[e][1]]) for e in odd]
        for _, _, key, kw in redone:
            assert key == KEY and kw == {"registration_binning": binning, "overlap_tolerance": None, "pairwise_reg_func_kwargs": kwargs, "device": 0,
                                         "_bin_cache": cache, "overlap_bbox": "reference"}
        # the counters as the parent sets them: the named pairs on the reference's sequence, the kept ones on raw crops
        assert cache.reference_pairs == len(odd) and cache.raw_crops == len(edges) - len(odd)

    # ---- memo miss: all pairs run, the named ones are redone, the memo holds them ----
    cache = registration._BinCache()
    first = _batched(sims, edges, binning, None, kwargs, cache)
    assert len(stand_ins.calls) == 1 and stand_ins.calls[0]["edges"] == edges
    assert stand_ins.calls[0]["bin"] == [[1] * (3 - ndim) + [1, 2, 3][-ndim:]] * len(edges)
    check_redone(cache)
    assert [first[e]["transform"] for e in odd] == ["reference"] * len(odd) and [first[e]["quality"] for e in odd] == [1, 2, 3]
    assert all(isinstance(first[e]["transform"], np.ndarray) for e in keep)
    assert list(registration._KNIFE_MEMO.values()) == [odd] and next(iter(registration._KNIFE_MEMO))[0] == "mosaic"
    assert not [t for t in threading.enumerate() if t.name == "mvs-crop-length"]
    # ---- memo hit: only the kept pairs run ----
    del redone[:]
    monkeypatch.setattr(registration, "_reference_crop_differs", _must_not_ask)
    cache = registration._BinCache()
    second = _batched(sims, edges, binning, None, kwargs, cache)
    assert len(stand_ins.calls) == 2 and stand_ins.calls[1]["edges"] == [edges[e] for e in keep]
    assert stand_ins.calls[1]["ptrs"] == [stand_ins.calls[0]["ptrs"][e] for e in keep]
    check_redone(cache)
    assert [second[e]["transform"] for e in odd] == ["reference"] * len(odd)
    _assert_same_results([second[e] for e in keep], [first[e] for e in keep])
    assert list(registration._KNIFE_MEMO.values()) == [odd]
    # ---- the question switched off: every pair stays in the batch ----
    monkeypatch.setattr(registration, "_KNIFE_CHECK", [False])
    cache = registration._BinCache()
    third = _batched(sims, edges, binning, None, kwargs, cache)
    assert stand_ins.calls[2]["edges"] == edges and cache.reference_pairs == 0 and cache.raw_crops == len(edges) and len(redone) == len(odd)
    _assert_same_results([third[e] for e in keep], [first[e] for e in keep])


def _must_not_ask(*a):
    raise AssertionError("the memo answers")


def test_driver_with_every_pair_on_the_knife_edge_runs_no_batch_on_a_memo_hit(monkeypatch, stand_ins):
    sims, edges, redone = _knife_setup(monkeypatch, np.random.default_rng(15), 2, _all_pairs(5))
    binning = {"y": 2, "x": 3}
    cache = registration._BinCache()
    first = _batched(sims, edges, binning, cache=cache)
    assert len(stand_ins.calls) == 1 and len(redone) == len(edges) and cache.reference_pairs == len(edges) and cache.raw_crops == 0
    cache = registration._BinCache()
    second = _batched(sims, edges, binning, cache=cache)
    assert len(stand_ins.calls) == 1 and len(redone) == 2 * len(edges) and cache.reference_pairs == len(edges) and cache.raw_crops == 0
    assert [r["transform"] for r in first + second] == ["reference"] * (2 * len(edges))


def test_driver_joins_the_crop_length_thread_when_the_run_raises(monkeypatch):
    # (the real question: some 20 ms of scipy on a thread that is still at work when the run fails at once)
    run = _RunRecorder(error=RuntimeError("the run failed"))
    monkeypatch.setattr(registration, "_run_pair_jobs", run)
    monkeypatch.setattr(registration, "_KNIFE_MEMO", {})
    monkeypatch.setattr(registration, "_KNIFE_CHECK", [True])
    sims = _mosaic(np.random.default_rng(16), 3, 5)
    with pytest.raises(RuntimeError, match="the run failed"):
        _batched(sims, _all_pairs(5), {"z": 1, "y": 1, "x": 1})
    assert len(run.calls) == 1
    assert not [t for t in threading.enumerate() if t.name == "mvs-crop-length"]
    assert not [k for k in registration._KNIFE_MEMO if k[0] == "mosaic"]      # an answer nobody waited for is not remembered


def test_driver_raises_for_a_pair_that_does_not_overlap(stand_ins):
    rng = np.random.default_rng(17)
    sims = _mosaic(rng, 2, 3)
    far = sims[2].attrs["transforms"][KEY].copy()
    far[:2, 2] += 1e4
    si.set_sim_affine(sims[2], far, KEY)
    with pytest.raises(ValueError, match="views do not overlap"):
        _batched(sims, [(0, 1), (1, 2)], {"y": 1, "x": 1})
    assert not stand_ins.calls
    assert not [t for t in threading.enumerate() if t.name == "mvs-crop-length"]
